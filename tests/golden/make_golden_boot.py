#!/usr/bin/env python
"""Generate tests/golden/boot_reference.npz: the reference's bootstrap of ESS / TFEP / mean free-energy estimates on seeded inputs.

    python tests/golden/make_golden_boot.py --reference /path/to/thermodynamic-interpolation

Only imports from the reference checkout (mdqm9/analysis/utils/free_energy.py, ess.py, sensititvity.py; the reference root goes on
sys.path because free_energy.py imports sensititvity through the package path) and records what its primitives return, composed as
the gen_* functions of mdqm9/analysis/results_00031.py compose them (that module imports rdkit and cannot be imported itself):

    none      (k=None)                 point on the sample; a resample = sample[choice(n, n)]
    once      (gen_ess_ti, gen_ess_bg) the sample is filtered once; a resample = filtered[choice(n_kept, n_kept)], not filtered again
    resample  (gen_free_energy_*)      point on the filtered sample; a resample = sample[choice(n_kept, n_kept)] -- the reference draws
                                       len(filtered) indices below len(filtered) over the UNFILTERED arrays -- filtered by its own quartiles

with phi = -logw fed in as (E0s = 0, E1s = phi, neg_dlogps = 0) / (Es = phi, neg_dlogps_bg = 0), which the reference's sums keep exact.
The index rows are those of np.random.RandomState(seed).choice, recorded.  Intervals are np.percentile(estimates, [2.5, 97.5]).

Guard (asserted): wherever a filter is applied -- the full sample and every recorded resample -- no value lies within relative 1e-9 of
a filter bound, so the kept sets do not depend on rounding.  A zero iqr is exempt: the bounds are then bit-equal to q25 whatever the
arithmetic and nothing is kept.  Seeds that miss the guard are skipped (the next one is tried); the seeds used are recorded.

Layout: per dataset d logw_flat[logw_off[d]:logw_off[d+1]] (fp32); per case c the columns case_* and idx_flat[idx_off[c]:idx_off[c+1]]
(uint16, [n_boot, n_draw] row-major), est_flat[est_off[c]:est_off[c+1]]."""
import argparse
import importlib
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ESS, TFEP, MEAN = 0, 1, 2
NONE, ONCE, RESAMPLE = 0, 1, 2
NS = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1000, 4097)
N_BOOT = {1: 3, 2: 3, 3: 4, 5: 5, 63: 8, 64: 8, 65: 8, 255: 8, 256: 8, 257: 16, 1000: 64, 4097: 6}
GUARD = 1e-9


class GuardMiss(Exception):
    pass


def heavy_tailed(seed, n):
    return np.clip(np.random.RandomState(seed).standard_normal(n) * 3.0, -30.0, 30.0).astype(np.float32)


class Reference:
    def __init__(self, root):
        sys.path.insert(0, root)
        self.fe = importlib.import_module("mdqm9.analysis.utils.free_energy")
        self.ess = importlib.import_module("mdqm9.analysis.utils.ess")
        self.sens = importlib.import_module("mdqm9.analysis.utils.sensititvity")

    def guard(self, x, k):
        if k is None or x.size == 0:
            return
        q75, q25 = np.percentile(x, [75, 25])
        iqr = q75 - q25
        if iqr == 0:
            return
        for b in (q25 - k * iqr, q75 + k * iqr):
            if (np.abs(x - b) <= GUARD * np.maximum(np.abs(x), abs(b))).any():
                raise GuardMiss()

    def filtered_x(self, phis, estimator):
        return phis if estimator == MEAN else np.exp(-phis)

    def estimate(self, phis, estimator, k):
        """(estimate, keep mask) of the reference's primitives on phis with filter multiple k (None: no filter)."""
        zero = np.zeros_like(phis)
        self.guard(self.filtered_x(phis, estimator), k)
        if estimator == ESS:                                   # gen_ess_ti
            weights = self.ess.calc_ti_weights(E0s=zero, E1s=phis, neg_dlogps_ti=zero)
            keep = self.sens.filter_iqr(weights, k=k)
            return self.ess.calc_ESS(weights[keep]), keep
        if estimator == TFEP:                                  # gen_free_energy_tfep_md_ti
            ph, keep = self.fe.calc_phis_tfep(E0s=zero, E1s=phis, neg_dlogps_ti=zero, k=k)
            return (self.fe.calc_tfep_dF(phis=ph, weights=np.ones_like(ph)) if ph.size else np.nan), keep
        keep = self.sens.filter_iqr(phis, k=k)                 # gen_free_energy_bg, one of its two samples
        ph = self.fe.calc_phis_bg(Es=phis, neg_dlogps_bg=zero, k=k)
        return (self.fe.calc_bg_dF(phis=ph) if ph.size else np.nan), keep

    def case(self, logw, estimator, mode, k, n_boot, seed):
        phis = -logw.astype(np.float64)
        kk = None if mode == NONE else k
        point, keep = self.estimate(phis, estimator, kk)
        kept = int(keep.sum())
        rs = np.random.RandomState(seed)
        pop = phis[keep] if mode == ONCE else phis
        idx = np.stack([rs.choice(np.arange(kept), kept, replace=True) for _ in range(n_boot)]) if kept else np.zeros((n_boot, 0), np.int64)
        est = np.full(n_boot, np.nan)
        for r in range(n_boot if kept else 0):
            est[r] = self.estimate(pop[idx[r]], estimator, k if mode == RESAMPLE else None)[0]
        lo, hi = (np.nan, np.nan) if np.isnan(est).any() else np.percentile(est, [2.5, 97.5])
        return dict(point=point, kept=kept, idx=idx, est=est, lo=lo, hi=hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TI_REFERENCE"), required=os.environ.get("TI_REFERENCE") is None)
    ap.add_argument("--out", default=os.path.join(HERE, "boot_reference.npz"))
    args = ap.parse_args()
    ref = Reference(args.reference)
    warnings.simplefilter("ignore")                            # the reference divides 0 / 0 on empty kept sets

    datasets, names = [], []

    def dataset(name, logw):
        names.append(name)
        datasets.append(np.asarray(logw, np.float32))
        return len(datasets) - 1

    plan = []                                                  # (dataset, estimator, mode, k, n_boot)
    combos = [(e, m, k) for e in (ESS, TFEP, MEAN) for m in (NONE, ONCE, RESAMPLE) for k in ((1.5,) if m == NONE else (1.5, 100.0))]
    for n in NS:
        d = dataset(f"n{n}", heavy_tailed(1000 + n, n))
        if n <= 65:
            todo = combos
        elif n <= 257:                                         # every estimator x mode, k alternating
            todo = [(e, m, (1.5, 100.0)[(e + m + n) % 2]) for e in (ESS, TFEP, MEAN) for m in (NONE, ONCE, RESAMPLE)]
        elif n == 1000:
            todo = [(ESS, ONCE, 100.0), (TFEP, RESAMPLE, 100.0), (MEAN, RESAMPLE, 1.5)]
        else:
            todo = [(ESS, ONCE, 1.5), (TFEP, RESAMPLE, 1.5), (MEAN, NONE, 1.5)]
        for i, (e, m, k) in enumerate(todo):
            plan.append((d, e, m, k, N_BOOT[n] if (n != 1000 or i == 0) else 8))
    dq = dataset("quantised_n300", np.round(heavy_tailed(77, 300) * 2.0) / 2.0)      # steps of 0.5: many ties at the quartiles
    dc = dataset("constant_n40", np.full(40, -1.25, np.float32))
    for d in (dq, dc):
        for e, m, k in [(ESS, ONCE, 1.5), (TFEP, RESAMPLE, 1.5), (MEAN, RESAMPLE, 1.5), (TFEP, NONE, 1.5), (ESS, RESAMPLE, 100.0)]:
            plan.append((d, e, m, k, 6))

    cols = {c: [] for c in ("data", "estimator", "mode", "k", "n_boot", "n_draw", "kept", "point", "lo", "hi", "seed")}
    idx_flat, est_flat, idx_off, est_off = [], [], [0], [0]
    for c, (d, e, m, k, nb) in enumerate(plan):
        seed = 5000 + 10 * c
        while True:
            try:
                r = ref.case(datasets[d], e, m, k, nb, seed)
                break
            except GuardMiss:
                seed += 1
                assert seed < 5000 + 10 * c + 10, ("no seed meets the guard", names[d], e, m, k)
        for key, v in dict(data=d, estimator=e, mode=m, k=k, n_boot=nb, n_draw=r["idx"].shape[1], kept=r["kept"], point=r["point"], lo=r["lo"],
                           hi=r["hi"], seed=seed).items():
            cols[key].append(v)
        assert r["idx"].size == 0 or r["idx"].max() < 65536
        idx_flat.append(r["idx"].astype(np.uint16).reshape(-1))
        est_flat.append(r["est"])
        idx_off.append(idx_off[-1] + r["idx"].size)
        est_off.append(est_off[-1] + nb)

    n_of = np.array([datasets[d].size for d in cols["data"]])
    n_draw, mode = np.array(cols["n_draw"]), np.array(cols["mode"])
    quirk = (mode == RESAMPLE) & (n_draw != n_of) & (n_draw > 0)
    assert quirk.any(), "no case reproduces the reference drawing len(filtered) indices over the unfiltered arrays"
    assert all(np.abs(ds).max() <= 30.0 for ds in datasets)
    np.savez_compressed(
        args.out, names=np.array(names), logw_flat=np.concatenate(datasets), logw_off=np.cumsum([0] + [ds.size for ds in datasets]),
        idx_flat=np.concatenate(idx_flat), idx_off=np.array(idx_off), est_flat=np.concatenate(est_flat), est_off=np.array(est_off),
        **{"case_" + key: np.array(v, np.float64 if key in ("k", "point", "lo", "hi") else np.int64) for key, v in cols.items()})
    est = np.concatenate(est_flat)
    print(f"{len(plan)} cases over {len(datasets)} datasets; {int(np.isnan(est).sum())} NaN estimates of {est.size}; "
          f"{int(quirk.sum())} cases with n_draw != n (e.g. case {int(np.argmax(quirk))}: n = {n_of[np.argmax(quirk)]}, n_draw = {n_draw[np.argmax(quirk)]}); "
          f"{os.path.getsize(args.out)} bytes")

    # the numpy restatement against what was just recorded
    sys.path.insert(0, os.path.dirname(HERE))
    import boot_numpy as bn
    worst = 0.0
    for c, (d, e, m, k, nb) in enumerate(plan):
        idx = np.concatenate(idx_flat)[idx_off[c]:idx_off[c + 1]].reshape(nb, -1).astype(np.int32)
        got = bn.bootstrap(datasets[d], e, m, k, 0.95, nb, indices=idx if idx.shape[1] else None)
        ref_est = est_flat[c]
        assert got[3] == cols["kept"][c] and (np.isnan(got[4]) == np.isnan(ref_est)).all(), c
        scale = 1 + (np.abs(datasets[d]).max() if e == MEAN else np.abs(np.nan_to_num(ref_est)))
        worst = max(worst, np.nanmax(np.abs(got[4] - ref_est) / (8 * max(idx.shape[1], 1) * 2.0 ** -53 * scale), initial=0.0))
    print(f"restatement vs reference, worst error as a fraction of 8 n_draw 2^-53 (1 + |ref|): {worst:.3f}")


if __name__ == "__main__":
    main()
