#!/usr/bin/env python
"""Measure the observables layer at the headline shape (65 536 molecules x 18 atoms, F = 128, L = 5, f16x2) on device tensors:
  1. one ti_obs_cv call, RMSD + 3 torsions;
  2. a 20-step Euler rollout (save_every = 0) with an observer at every = 1 against the same rollout without it;
  3. the device-to-host copy of one [B, 18, 3] fp32 row (216 B per molecule) that a CV row replaces, pageable and pinned.
Medians of --reps timed calls after one warm-up, wall clock around synchronous library calls.  Prints one JSON line.

    python tools/obs_bench.py [--batch 65536] [--reps 7]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    import torch
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    syn, W = ti.synthetic, ti.weights
    F, L, A, B = 128, 5, 18, args.batch
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=0), W.painn_param_spec(0, F, L, 25))
    eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision="f16x2")
    x0h, condh = syn.molecule_coords(B, A, seed=11), syn.ambient_cond(B, A)
    x0, cond = torch.from_numpy(x0h).cuda(), torch.from_numpy(condh).cuda()
    desc = [("rmsd",), ("torsion", 0, 1, 2, 3), ("torsion", 4, 5, 6, 7), ("torsion", 8, 9, 10, 11)]
    ref = x0h[0]
    cv = torch.empty((B, len(desc)), device="cuda")
    sync = torch.cuda.synchronize
    rec = {"shape": f"{B} x {A}", "F": F, "L": L, "precision": "f16x2", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    rec["obs_cv_ms"], rec["obs_cv_ms_min"] = median_ms(lambda: eng.collective_variables(x0, desc, ref=ref, out=cv), args.reps)

    grid = ti.engine.time_grid(0.0, 1.0, args.steps + 1)
    out = torch.empty((1, B, A, 3), device="cuda")
    roll = lambda: eng.rollout(x0, cond, grid, scheme="euler", save_every=0, out=out)
    rec["rollout_ms"], rec["rollout_ms_min"] = median_ms(roll, args.reps)
    plain = out.clone()
    rows = args.steps + 1
    cvs = torch.empty((rows, B, len(desc)), device="cuda")
    eng.set_observer(desc, ref=ref, every=1, out=cvs)
    rec["rollout_observed_ms"], rec["rollout_observed_ms_min"] = median_ms(roll, args.reps)
    eng.set_observer(None)
    rec["end_state_bit_identical"] = bool(torch.equal(plain.view(torch.int32), out.view(torch.int32)))
    rec["observer_ms_per_row"] = (rec["rollout_observed_ms"] - rec["rollout_ms"]) / rows
    rec["observer_overhead_pct"] = 100.0 * (rec["rollout_observed_ms"] - rec["rollout_ms"]) / rec["rollout_ms"]

    host = np.empty((B, A, 3), np.float32)
    pinned = torch.empty((B, A, 3), pin_memory=True)

    def d2h_pageable():
        host[...] = x0.cpu().numpy()

    def d2h_pinned():
        pinned.copy_(x0, non_blocking=True)
        sync()

    rec["row_bytes"] = int(x0.numel() * 4)
    rec["cv_row_bytes"] = int(B * len(desc) * 4)
    rec["d2h_row_pageable_ms"], _ = median_ms(d2h_pageable, args.reps)
    rec["d2h_row_pinned_ms"], _ = median_ms(d2h_pinned, args.reps)
    cvp = torch.empty((B, len(desc)), pin_memory=True)

    def d2h_cv():
        cvp.copy_(cv, non_blocking=True)
        sync()

    rec["d2h_cv_row_pinned_ms"], _ = median_ms(d2h_cv, args.reps)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
