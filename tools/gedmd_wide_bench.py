#!/usr/bin/env python
"""Measure gEDMD at the molecule study's size: the blocked Gram pass (ti_obs_rff_gram_wide), the bootstrapped generator spectrum around
it and the cross-validated score, against the reference's SVD route in numpy on the same machine's CPU.

Shapes: n = 25 000 and n = 100 000 torsion-like samples (d = 6, fp32, wrapped to (-pi, pi], a device tensor), p = 300 Gaussian features
(sigma = 5), nev = 4, tol = 1e-4, a = k_B 300 K, 1000 resamples -- the call of the reference's mdqm9/analysis/gedmd.py.
GPU, wall clock:
  gram       observables.rff_gram_wide alone (the 1001 Gram matrices stay on the device; the call is synchronous): median of --reps
             calls after one warm-up
  generator  observables.gedmd_generator: the same call, the copy of the Gram matrices to the host, and the host eigh stage
  host       observables.gedmd_spectrum alone on the copied Gram matrices -- its share of `generator` is printed
             (two eigh calls of order ~300 per resample take tens of seconds a pass, so these two are medians of --algebra-reps calls,
             default 1, without a warm-up)
  cv         one observables.gedmd_cv (20 splits, 75 / 25) at p = 300 and one at p = 1000 on the first size, with the share of its two
             Gram calls
CPU: tests/gedmd_numpy.py svd_route -- the reference's algorithm, an SVD of the [p, m] feature matrix per resample -- timed over
--cpu-resamples resamples and scaled to 1000: the loop is linear in the resamples.
The Gram pass's arithmetic per call: 4 MFMAs of 2 * 16 * 16 * 4 flop per upper-triangle tile and 4 draws; its gathered bytes: a diagonal
panel pair reads its panel's 2 * 8 * 16 columns per draw, an off-diagonal pair both panels'.
  wide       the blocked device route: observables.gedmd_spectrum_wide alone on the Gram stack where it lies (the spectrum stage) and
             observables.gedmd_generator_wide (the whole call), medians of --wide-reps calls after one warm-up, with the largest
             difference of their spectra from the host route's (--wide-reps 0 leaves the stage out)
--gram-only: two Gram calls per size and nothing else (the run to put under rocprofv3 --kernel-trace --stats).
--spectrum-only: one Gram call and two gedmd_spectrum_wide calls per size and nothing else (the same, for the blocked solver's kernels).
Prints one JSON line per size and one per cv.

    python tools/gedmd_wide_bench.py [--reps 7] [--algebra-reps 1] [--wide-reps 7] [--cpu-resamples 3] [--gram-only | --spectrum-only]
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


def timed_ms(fn, reps, warm):
    if warm:
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def samples(n, d, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((n, d))
    x[:, 0] = np.where(rs.random_sample(n) < 0.5, -1.0, 1.0) + 0.35 * x[:, 0]
    return (np.pi - np.mod(np.pi - 1.5 * x, 2 * np.pi)).astype(np.float32)


def gathered_columns(T):
    """doubles gathered per draw over all panel pairs: 2 (cos, sin) x 16 columns x the tiles of the pair's panels"""
    w = [8] * (T // 8) + ([T % 8] if T % 8 else [])
    return 32 * sum(w[i] if i == j else w[i] + w[j] for i in range(len(w)) for j in range(i, len(w)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--algebra-reps", type=int, default=1)
    ap.add_argument("--resamples", type=int, default=1000)
    ap.add_argument("--cpu-resamples", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[25000, 100000])
    ap.add_argument("--p", type=int, default=300)
    ap.add_argument("--cv-ps", type=int, nargs="*", default=[300, 1000])
    ap.add_argument("--wide-reps", type=int, default=7)
    ap.add_argument("--gram-only", action="store_true")
    ap.add_argument("--spectrum-only", action="store_true")
    args = ap.parse_args()
    import torch
    import gedmd_numpy as gn
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    obs = ti.observables
    eng = obs._service_engine(0)
    d, p, nev, a, tol, nb, sigma = 6, args.p, 4, 0.008314462618 * 300.0, 1e-4, args.resamples, 5.0
    omega = obs.sample_rff_gaussian(d, p, sigma, 0)
    T = -(-p // 16)
    for n in args.sizes:
        x = samples(n, d, n)
        dev = torch.from_numpy(x).cuda()
        if args.gram_only:
            for _ in range(2):
                obs.rff_gram_wide(dev, omega, n_boot=nb, seed=1, engine=eng)
            continue
        if args.spectrum_only:
            G = obs.rff_gram_wide(dev, omega, n_boot=nb, seed=1, engine=eng)
            for _ in range(2):
                obs.gedmd_spectrum_wide(G, omega, a, nev, tol, engine=eng)
            continue
        gram_ms, gram_min = timed_ms(lambda: obs.rff_gram_wide(dev, omega, n_boot=nb, seed=1, engine=eng), args.reps, True)
        flop = (n * (1 + nb) / 4) * (T * (T + 1) / 2) * 4 * 2 * 16 * 16 * 4
        rec = dict(n=n, d=d, p=p, resamples=nb, gram_ms=gram_ms, gram_ms_min=gram_min, gram_call_tflops=flop / (gram_ms * 1e-3) / 1e12,
                   gram_call_gather_GBps=n * (1 + nb) * 8 * gathered_columns(T) / (gram_ms * 1e-3) / 1e9)
        print(json.dumps(dict(rec, stage="gram")), flush=True)
        res = []
        gen_ms, _ = timed_ms(lambda: res.append(obs.gedmd_generator(dev, omega, nev, a, tol=tol, n_boot=nb, seed=1, engine=eng)), args.algebra_reps, False)
        G = obs.rff_gram_wide(dev, omega, n_boot=nb, seed=1, engine=eng).cpu().numpy()
        host = []
        host_ms, _ = timed_ms(lambda: host.append(obs.gedmd_spectrum(G, omega, a, nev, tol)), args.algebra_reps, False)
        if args.wide_reps > 0:
            host_d = host[-1][0]
            Gd, wide = obs.rff_gram_wide(dev, omega, n_boot=nb, seed=1, engine=eng), []
            spec_ms, spec_min = timed_ms(lambda: wide.append(obs.gedmd_spectrum_wide(Gd, omega, a, nev, tol, engine=eng)), args.wide_reps, True)
            del Gd
            wgen_ms, wgen_min = timed_ms(lambda: obs.gedmd_generator_wide(dev, omega, nev, a, tol=tol, n_boot=nb, seed=1, engine=eng),
                                         args.wide_reps, True)
            rec.update(wide_spectrum_ms=spec_ms, wide_spectrum_ms_min=spec_min, wide_generator_ms=wgen_ms, wide_generator_ms_min=wgen_min,
                       wide_reps=args.wide_reps, wide_against_host=float(np.abs(wide[-1][0] - host_d).max()),
                       wide_ranks=[int(wide[-1][2].min()), int(wide[-1][2].max())], speedup_spectrum=host_ms / spec_ms,
                       speedup_wide_generator=gen_ms / wgen_ms)
        del G
        c, ref = [], [np.full(nev, np.nan)]
        if args.cpu_resamples > 0:
            rr = np.random.RandomState(1)
            t0 = time.perf_counter()
            for _ in range(args.cpu_resamples):
                ref = gn.svd_route(x[rr.choice(n, n)], omega, a, nev, tol)
            c.append((time.perf_counter() - t0) * 1e3 * nb / args.cpu_resamples)
        rec.update(generator_ms=gen_ms, host_eigh_ms=host_ms, host_share=host_ms / gen_ms, algebra_reps=args.algebra_reps,
                   cpu_numpy_ms=c[0] if c else None, cpu_resamples_timed=args.cpu_resamples, speedup_generator=c[0] / gen_ms if c else None,
                   eigenvalues=res[-1].eigenvalues.tolist(), ci=res[-1].ci.tolist(), rank=res[-1].rank, cpu_last_resample=ref[0].tolist(),
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
    if args.gram_only or args.spectrum_only:
        return
    n = args.sizes[0]
    dev = torch.from_numpy(samples(n, d, n)).cuda()
    for pc in args.cv_ps:
        om = obs.sample_rff_gaussian(d, pc, sigma, 0)
        perms = np.stack([np.random.RandomState(r).permutation(n) for r in range(20)]).astype(np.int32)
        idx = [torch.from_numpy(np.ascontiguousarray(h)).cuda() for h in (perms[:, :int(0.75 * n)], perms[:, int(0.75 * n):])]
        grams_ms, _ = timed_ms(lambda: [obs.rff_gram_wide(dev, om, n_boot=20, indices=i, engine=eng) for i in idx], 1, True)
        out = []
        cv_ms, _ = timed_ms(lambda: out.append(obs.gedmd_cv(dev, om, a, nev, tol, splits=perms, engine=eng)), 1, False)
        print(json.dumps(dict(stage="cv", n=n, d=d, p=pc, splits=20, cv_ms=cv_ms, gram_calls_ms=grams_ms, gram_share=grams_ms / cv_ms,
                              mean_score=float(np.mean(out[0].scores)), ranks=[int(out[0].rank.min()), int(out[0].rank.max())])), flush=True)


if __name__ == "__main__":
    main()
