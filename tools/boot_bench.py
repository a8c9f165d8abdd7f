#!/usr/bin/env python
"""Measure ti_obs_bootstrap against the reference's loop in numpy on the same machine's CPU.

Shapes: n = 65 536 and n = 400 000 samples (logw ~ 3 N(0, 1), fp32, a device tensor), 1000 resamples, for
  ess_once       ESS, the sample filtered once, k = 100                 (gen_ess_ti)
  tfep_resample  TFEP, every resample filtered by its own quartiles, k = 100   (gen_free_energy_tfep_md_ti)
  tfep_none      TFEP without a filter
GPU: median of --reps calls after one warm-up, wall clock around the synchronous library call (estimates stay on the device).
CPU: tests/boot_numpy.py reference_loop -- the reference's algorithm with RandomState.choice and np.percentile -- timed over
--cpu-resamples resamples (median of 3) and scaled to 1000: the loop's cost is linear in the resamples, and the full loop takes
minutes at the larger size.  Prints one JSON line per case.

    python tools/boot_bench.py [--reps 7] [--cpu-resamples 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--resamples", type=int, default=1000)
    ap.add_argument("--cpu-resamples", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 400000])
    args = ap.parse_args()
    import torch
    import boot_numpy as bn
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    eng = ti.observables._service_engine(0)
    cases = [("ess_once", bn.ESS, bn.ONCE, 100.0), ("tfep_resample", bn.TFEP, bn.RESAMPLE, 100.0), ("tfep_none", bn.TFEP, bn.NONE, 1.0)]
    for n in args.sizes:
        logw = (np.random.RandomState(n).standard_normal(n) * 3.0).astype(np.float32)
        dev = torch.from_numpy(logw).cuda()
        out = torch.empty(args.resamples, dtype=torch.float64, device="cuda")
        for name, est, mode, k in cases:
            call = lambda: eng.bootstrap(dev, est, mode, k, 0.95, args.resamples, 0, 1, None, out_boot=out)
            res = call()
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                t.append((time.perf_counter() - t0) * 1e3)
            c = []
            for _ in range(3):
                t0 = time.perf_counter()
                ref = bn.reference_loop(logw, est, mode, k, args.cpu_resamples, np.random.RandomState(1))
                c.append((time.perf_counter() - t0) * 1e3 * args.resamples / args.cpu_resamples)
            rec = dict(case=name, n=n, resamples=args.resamples, gpu_ms=float(np.median(t)), gpu_ms_min=float(np.min(t)),
                       cpu_numpy_ms=float(np.median(c)), cpu_resamples_timed=args.cpu_resamples, speedup=float(np.median(c) / np.median(t)),
                       point=res[0], ci=[res[1], res[2]], n_kept=res[3], cpu_point=float(ref[0]), device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
