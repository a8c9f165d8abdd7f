#!/usr/bin/env python3
"""What replica exchange (ti_obs_ff_remd) costs over plain Langevin dynamics (ti_obs_ff_langevin) in the same session: the launch
cut at every attempt and the two force evaluations of a pair.  tools/md_bench.py's species (synthetic A = 9 and A = 25, relaxed the
same way) and sizes: 8 rungs 300 .. 1000 K x 128 ladders = 1024 rows, dt = 1 fs, friction = 1 / ps, state in device memory, no
frames; 4000 steps a call, exchange_every in {10, 100, 1000}.
    timeout -k 10 300 python tools/remd_bench.py [repeats=5]
Reported: microseconds per step of the whole batch -- the quantity of profiles/md_bench.txt's "us per step" -- as the median of
the repeats after a warm-up call, with min and max, and the ratio to the plain run."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from md_bench import DT, FRICTION, relax, timed  # noqa: E402

K, LADDERS, N_STEPS, EVERY = 8, 128, 4000, (10, 100, 1000)


def main():
    reps = max(int(sys.argv[1]) if len(sys.argv) > 1 else 5, 3)
    import torch
    import ff_numpy as fn
    import ff_forces_numpy as ffn
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    syn, W, E = ti.synthetic, ti.weights, ti.engine
    B = K * LADDERS
    temps = np.tile(np.arange(300, 1001, 100).astype(np.float32), LADDERS)                   # ladder-major: row l K + k is rung k
    results = []
    for A in (9, 25):
        ffd = fn.synthetic_forcefield(A)
        flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, 32, 1, 25, 0), W.painn_param_spec(W.AMBIENT, 32, 1, 25))
        eng = E.PainnEngine(W.AMBIENT, 32, 1, A, *syn.fully_connected_template(A), np.arange(A), flat, temp_length=100.0)
        eng.set_forcefield(ti.forcefield.ForceField(**ffd, masses=ffn.masses_for(ffd)))
        base, to_nm = fn.synthetic_geometry(ffd, 64, seed=1)
        pos = torch.from_numpy(base[np.arange(B) % len(base)].astype(np.float64) * to_nm).cuda()
        pos, dt_reached = relax(ti, eng, pos)
        T = torch.from_numpy(temps).cuda()
        pos, vel, _, _, _ = eng.langevin(pos, None, T, DT, FRICTION, 2000, seed=2, draw_velocities=True)
        state = [pos, vel, 2000, None]

        def plain():
            p, v, _, _, _ = eng.langevin(state[0], state[1], T, DT, FRICTION, N_STEPS, seed=2, step_offset=state[2])
            state[0], state[1], state[2] = p, v, state[2] + N_STEPS

        def exchange(every, tally):
            p, v, _, _, _, w, _, cnt = eng.remd(state[0], state[1], T, K, every, DT, FRICTION, N_STEPS, seed=2, step_offset=state[2], walker=state[3])
            state[0], state[1], state[2], state[3] = p, v, state[2] + N_STEPS, w
            tally += cnt.sum(dim=(0, 1)).cpu().numpy()

        t0, lo0, hi0 = timed(plain, reps)
        print(f"A = {A}, {K} rungs x {LADDERS} ladders, {N_STEPS} steps, no frames (relaxed to a step of {dt_reached * 1e3:.3g} fs first)")
        print(f"  ti_obs_ff_langevin:                median of {reps} {t0 * 1e3:8.2f} ms (min {lo0 * 1e3:.2f}, max {hi0 * 1e3:.2f}) = {t0 / N_STEPS * 1e6:6.2f} us per step")
        r = dict(atoms=A, rows=B, steps=N_STEPS, langevin_us_per_step=t0 / N_STEPS * 1e6, remd={})
        for every in EVERY:
            tally = np.zeros(2, np.int64)
            t, lo, hi = timed(lambda: exchange(every, tally), reps)
            print(f"  ti_obs_ff_remd, exchange_every {every:4d}: median of {reps} {t * 1e3:8.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f}) = {t / N_STEPS * 1e6:6.2f} us per step, "
                  f"{t / t0:.3f} of plain, {(t - t0) / (N_STEPS // every) * 1e6:.1f} us per attempt; accepted {tally[1]} of {tally[0]}")
            r["remd"][every] = dict(us_per_step=t / N_STEPS * 1e6, ratio=t / t0, us_per_attempt=(t - t0) / (N_STEPS // every) * 1e6,
                                    attempts=int(tally[0]), accepted=int(tally[1]))
        results.append(r)
    print(json.dumps({"workload": "replica exchange against plain Langevin dynamics, synthetic species, 8 rungs x 128 ladders, dt = 1 fs, "
                                  "friction = 1 / ps, device memory, no frames", "results": results}))


if __name__ == "__main__":
    main()
