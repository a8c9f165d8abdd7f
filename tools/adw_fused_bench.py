#!/usr/bin/env python3
"""Fused against unfused adw rollout, same build, same box, interleaved.
    python tools/adw_fused_bench.py [--repeats 3] [--out FILE] [--only large|small] [--precisions f32,f16x2] [--one-fused SHAPE]
H = 256, 5 layers, device tensors, end state only (save_every = 0).  Shapes:
  large_em     B = 262 144, 1 001-point grid, EM eps = 0.01          (bench_extra.py --which adw)
  large_dlogp  B = 262 144, 1 001-point grid, Euler with dlogp
  b512_dlogp   B = 512,     400-point grid,   Euler with dlogp       (the reference config's batch and n_step)
  b4096_dlogp  B = 4 096,   400-point grid,   Euler with dlogp
Every timed call ends in a device synchronise; fused and unfused alternate, `repeats` each, after one warm-up call of each.  One
JSON line per (shape, precision): medians, min..max spreads, ms per step, the ratio, and whether the two results are bit-identical.
--one-fused SHAPE runs a single fused call of that shape and nothing else (for a kernel trace)."""
import argparse
import importlib
import json
import os
import sys
import time

SHAPES = {"large_em": (262144, 1001, dict(scheme="em", eps=0.01, seed=1)),
          "large_dlogp": (262144, 1001, dict(scheme="euler", return_dlogp=True)),
          "b512_dlogp": (512, 400, dict(scheme="euler", return_dlogp=True)),
          "b4096_dlogp": (4096, 400, dict(scheme="euler", return_dlogp=True))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("large", "small"), default=None)
    ap.add_argument("--precisions", default="f32,f16x2")
    ap.add_argument("--one-fused", default=None, choices=sorted(SHAPES))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    syn, W = ti.synthetic, ti.weights
    H, L = 256, 5
    flat = W.flatten_state_dict(syn.adw_state_dict(H, L, 0), W.adw_param_spec(H, L), dtype=np.float64)
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    def inputs(B):
        gen = torch.Generator(device="cuda").manual_seed(0)
        return torch.randn((B,), device="cuda", generator=gen), torch.full((B,), 1.0, device="cuda"), torch.full((B,), 1.25, device="cuda")

    if a.one_fused:
        B, n, kw = SHAPES[a.one_fused]
        eng = ti.engine.AdwEngine(H, L, flat, precision=a.precisions.split(",")[0])
        x, b0, b1 = inputs(B)
        eng.rollout(x, b0, b1, ti.engine.time_grid(0.0, 1.0, n), save_every=0, fused=True, **kw)
        torch.cuda.synchronize()
        return
    names = [s for s in SHAPES if a.only is None or s.startswith("large") == (a.only == "large")]
    for prec in a.precisions.split(","):
        eng = ti.engine.AdwEngine(H, L, flat, precision=prec)
        for name in names:
            B, n, kw = SHAPES[name]
            grid = ti.engine.time_grid(0.0, 1.0, n)
            x, b0, b1 = inputs(B)

            def run(fused):
                t0 = time.perf_counter()
                res = eng.rollout(x, b0, b1, grid, save_every=0, fused=fused, **kw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, res
            last = {f: run(f)[1] for f in (False, True)}                    # warm-up: workspaces, code objects
            times = {False: [], True: []}
            for _ in range(a.repeats):
                for f in (False, True):
                    dt, last[f] = run(f)
                    times[f].append(dt)
            same = all(bool(torch.equal(u, v)) for u, v in zip(last[False][:-1], last[True][:-1])) and last[False][-1] == last[True][-1]
            med = {f: sorted(times[f])[len(times[f]) // 2] for f in times}
            emit(dict(shape=name, precision=prec, H=H, L=L, B=B, n_step=n, repeats=a.repeats, bit_identical=same,
                      unfused_s=round(med[False], 5), unfused_min_max_s=[round(min(times[False]), 5), round(max(times[False]), 5)],
                      fused_s=round(med[True], 5), fused_min_max_s=[round(min(times[True]), 5), round(max(times[True]), 5)],
                      unfused_ms_per_step=round(1e3 * med[False] / (n - 1), 4), fused_ms_per_step=round(1e3 * med[True] / (n - 1), 4),
                      unfused_over_fused=round(med[False] / med[True], 3)))
        del eng
    if out:
        out.close()


if __name__ == "__main__":
    main()
