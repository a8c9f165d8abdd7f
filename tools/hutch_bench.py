#!/usr/bin/env python3
"""Hutchinson estimator vs exact divergence at the headline shape (F = 128, L = 5, A = 18), torch-free.
    python tools/hutch_bench.py [molecules=2048] [repeats=3] [noise_molecules=512]
One JSON line per (precision, exact | k): molecule-evaluations/s of drift + divergence.  Then the noise the estimator buys: the std
over molecules of (Hutchinson - exact) end-of-rollout dlogp of a 20-step Heun run (ambient scales: div 1e-2, dlogp * 1e2), next to
the typical |dlogp|."""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

KS = (1, 4, 16)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    Bn = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    syn, W, E = ti.synthetic, ti.weights, ti.engine
    F, L, A = 128, 5, 18
    tpl = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, F, L, 25, 0), W.painn_param_spec(W.AMBIENT, F, L, 25))
    x, cond = syn.molecule_coords(B, A, seed=0), syn.ambient_cond(B, A)
    for prec in ("f16x2", "f32"):
        eng = E.PainnEngine(W.AMBIENT, F, L, A, *tpl, np.arange(A), flat, temp_length=100.0, precision=prec)
        base = None
        for k in (None,) + KS:
            call = (lambda: eng.drift_div(x, 0.5, cond)) if k is None else (lambda: eng.drift_div_est(x, 0.5, cond, n_probes=k))
            call()                                                    # warm-up (workspace allocation)
            t0 = time.perf_counter()
            for _ in range(reps):
                _, div = call()
            dt = (time.perf_counter() - t0) / reps
            base = base or dt
            print(json.dumps({"workload": f"drift + {'exact divergence' if k is None else f'Hutchinson k={k}'}, {B} molecules, F=128 L=5 A=18",
                              "precision": prec, "divergence": "exact" if k is None else "hutchinson", "n_probes": k,
                              "molecule_evaluations_per_s": B / dt, "ms_per_evaluation": dt * 1e3, "speedup_vs_exact": base / dt,
                              "finite": bool(np.isfinite(div).all())}), flush=True)
        eng.close()
    # noise: end-of-rollout dlogp of a 20-step Heun run, f16x2
    eng = E.PainnEngine(W.AMBIENT, F, L, A, *tpl, np.arange(A), flat, temp_length=100.0, precision="f16x2")
    grid = E.time_grid(0.0, 1.0, 21)
    kw = dict(scheme="heun", save_every=0, div_scale=1e-2, out_scale=1e2)
    _, dl_x, _ = eng.rollout_dlogp(x[:Bn], cond[:Bn], grid, **kw)
    for k in KS:
        _, dl_h, _ = eng.rollout_dlogp_est(x[:Bn], cond[:Bn], grid, n_probes=k, probe_seed=1, **kw)
        d = (dl_h[-1] - dl_x[-1]).astype(np.float64)
        print(json.dumps({"workload": f"20-step Heun dlogp, {Bn} molecules, F=128 L=5 A=18, f16x2", "n_probes": k,
                          "std_hutchinson_minus_exact": float(d.std()), "mean_hutchinson_minus_exact": float(d.mean()),
                          "mean_abs_exact_dlogp": float(np.abs(dl_x[-1]).mean()), "std_exact_dlogp": float(dl_x[-1].std())}), flush=True)


if __name__ == "__main__":
    main()
