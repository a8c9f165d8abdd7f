#!/usr/bin/env python3
"""FCNetMultiBeta(d, d, H, L) throughput: particle-steps/s at H = 256, 5 layers, B = 262 144 for d in {1, 2, 3, 8, 16}, f32 and f16x2.
    python tools/adw_nd_bench.py [--root DIR] [--dims 1,2,3,8,16] [--B 262144] [--steps 8] [--repeats 3]
Two workloads on device-resident tensors, end state only (save_every = 0): EM drift only (eps = 0.1), and Euler with the dlogp
state (exact divergence, d forward-mode directions).  One JSON line per (workload, precision, d) with the median over repeats.
--root DIR imports the package from another checkout (the d = 1 A/B against earlier sources, which know no d > 1)."""
import argparse
import importlib
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--dims", default="1,2,3,8,16")
    ap.add_argument("--B", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precisions", default="f32,f16x2")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    syn, W = ti.synthetic, ti.weights
    H, L, B = 256, 5, a.B
    grid = np.linspace(0.0, 1.0, a.steps + 1).astype(np.float32)
    b0 = torch.full((B,), 1.0, device="cuda")
    b1 = torch.full((B,), 1.25, device="cuda")
    for d in [int(v) for v in a.dims.split(",")]:
        spec = W.adw_param_spec(H, L, d, d)
        flat = W.flatten_state_dict(syn.make_state_dict(spec, seed=0, dtype=np.float64), spec, dtype=np.float64)
        gen = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn((B,) if d == 1 else (B, d), device="cuda", generator=gen)
        for prec in a.precisions.split(","):
            kw = dict(precision=prec) if d == 1 else dict(precision=prec, dim=d)
            eng = ti.engine.AdwEngine(H, L, flat, **kw)
            for work, rk in (("em_drift", dict(scheme="em", eps=0.1, seed=1)), ("euler_dlogp", dict(scheme="euler", return_dlogp=True))):
                eng.rollout(x, b0, b1, grid, save_every=0, **rk)                   # warm-up: workspaces, code objects
                torch.cuda.synchronize()
                times = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    res = eng.rollout(x, b0, b1, grid, save_every=0, **rk)
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                assert bool(torch.isfinite(res[0]).all())
                dt = sorted(times)[len(times) // 2]
                print(json.dumps(dict(workload=work, precision=prec, d=d, H=H, L=L, B=B, steps=a.steps,
                                      seconds=round(dt, 5), particle_steps_per_s=round(B * a.steps / dt, 1),
                                      ms_per_step=round(1e3 * dt / a.steps, 4))), flush=True)
            del eng


if __name__ == "__main__":
    main()
