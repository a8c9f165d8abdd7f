#!/usr/bin/env python
"""Measure TICA at the molecule study's size (ti_obs_tica_moments, ti_obs_tica_fit, ti_obs_tica_transform) against the numpy
restatement of the same three stages (tests/tica_numpy.py) on the same machine's CPU.

Size: K = 22 torsions (d = 44), the 11 lags of the reference's mdqm9/plots/10506_main.ipynb (1, 2, 4, .., 512, 1000), dim = 2,
1 000 000 frames in 8 trajectories of synthetic three-well torsions (``wells_fast``), fp32, a device tensor; the projection of 100 000 rows.
GPU: medians of --reps wall-clock calls after --warmup (the calls are synchronous):
  moments    engine.tica_moments (count, sum, cov stay on the device)
  fit        engine.tica_fit on those moments (mean, eigenvalues, components, rank stay on the device)
  transform  engine.tica_transform of the first 100 000 rows, all lags in one launch
CPU: the restatement's moments / fit / transform, one call each (--cpu-reps), numpy's threads as the environment sets them.
The moments kernel's arithmetic over the call's time, two ways: the flop of the definition, sum over the lags of N_tau d (3 d + 1), and the
flop the matrix cores execute, 2 * 256 per 16 x 16 tile and pair over the T (T + 1) + T^2 + 2 T tiles of a pair (T = d rounded up to 16,
over 16: the upper-triangle tiles of Sxx and Syy, all of Sxy, the two column sums; pad columns included).  Both are rates of the CALL
-- feature pass, table upload, reduce and synchronisation included; the contraction kernel's own time comes from a kernel trace of
this script in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/tica_bench.py --cpu-reps 0).  No
share of a peak is printed: no fp64 matrix rate of this part has been measured in this repository.  Prints one JSON line.

    python tools/tica_bench.py [--reps 7] [--warmup 2] [--frames 1000000] [--cpu-reps 1]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def wells_fast(K, n, n_traj, seed):
    """x [n, K] float32, traj_off: tn.synthetic's torsions with the three wells on a ring instead of a line, so that the walk is a
    cumulative sum and a million frames take a moment to draw (the generator of the tests walks frame by frame)"""
    import tica_numpy as tn
    rng = np.random.default_rng(seed)
    off = np.linspace(0, n, n_traj + 1).astype(np.int64)
    rate = np.minimum(0.002 * 3.0 ** np.arange(K), 0.4)
    x = np.empty((n, K), np.float32)
    for k in range(K):
        move = np.where(rng.random(n) < rate[k], np.where(rng.random(n) < 0.5, 1, 2), 0)
        move[off[:-1]] = rng.integers(0, 3, n_traj)                 # a fresh well at every trajectory start
        v = tn.WELLS[np.cumsum(move) % 3] + 0.3 * rng.standard_normal(n)
        x[:, k] = np.pi - np.mod(np.pi - v, 2.0 * np.pi)
    return x, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--cpu-reps", type=int, default=1)
    args = ap.parse_args()
    import torch
    import tica_numpy as tn
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    eng = ti.observables._service_engine(0)
    K, dim, n = 22, 2, args.frames
    d = 2 * K
    lags = np.array([2 ** i for i in range(10)] + [1000], np.int32)
    x, off = wells_fast(K, n, 8, 0)
    dev = torch.from_numpy(x).cuda()
    rows = dev[:args.rows]
    mom_ms, mom_min = median_ms(lambda: eng.tica_moments(dev, off, lags, 1), args.reps, args.warmup)
    count, sm, cov = eng.tica_moments(dev, off, lags, 1)
    fit_ms, fit_min = median_ms(lambda: eng.tica_fit(count, sm, cov, dim, 1e-6, 1), args.reps, args.warmup)
    mean, ev, comp, rank = eng.tica_fit(count, sm, cov, dim, 1e-6, 1)
    tr_ms, tr_min = median_ms(lambda: eng.tica_transform(rows, mean, comp, 1), args.reps, args.warmup)
    cpu = {}
    if args.cpu_reps > 0:
        t = []
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            rc, rs, rv = tn.moments(x, off, lags)
            t1 = time.perf_counter()
            model = [tn.fit(rc[l], rs[l], rv[l], dim) for l in range(len(lags))]
            t2 = time.perf_counter()
            for m in model:
                tn.transform(x[:args.rows], m[0], m[2])
            t3 = time.perf_counter()
            t.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        cm, cf, ct = (float(v) for v in np.median(np.array(t), axis=0))
        ev_off = float(np.abs(ev.cpu().numpy() - np.stack([m[1] for m in model])).max())
        cpu = dict(cpu_moments_ms=cm, cpu_fit_ms=cf, cpu_transform_ms=ct, speedup_moments=cm / mom_ms, speedup_fit=cf / fit_ms,
                   speedup_transform=ct / tr_ms, eigenvalues_off_by=ev_off, cpu_threads=os.environ.get("OMP_NUM_THREADS"))
    pairs = int(count.sum().item())
    T = -(-d // 16)
    flop, flop_exec = float(pairs) * d * (3 * d + 1), 512.0 * pairs * (T * (T + 1) + T * T + 2 * T)
    rec = dict(frames=n, trajectories=8, K=K, d=d, lags=lags.tolist(), dim=dim, rows=args.rows, pairs=pairs, moments_ms=mom_ms, moments_ms_min=mom_min,
               fit_ms=fit_ms, fit_ms_min=fit_min, transform_ms=tr_ms, transform_ms_min=tr_min, moments_call_tflops=flop / (mom_ms * 1e-3) / 1e12,
               moments_call_tflops_executed=flop_exec / (mom_ms * 1e-3) / 1e12,
               eigenvalues_lag1=ev[0].cpu().numpy().tolist(), rank=rank.cpu().numpy().tolist(), **cpu, device=torch.cuda.get_device_name(0))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
