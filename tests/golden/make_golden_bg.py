#!/usr/bin/env python
"""Generate tests/golden/bg_reference.npz: the reference's Boltzmann-generator weights on seeded inputs.

    python tests/golden/make_golden_bg.py --reference /path/to/thermodynamic-interpolation

Only imports from the reference checkout (mdqm9/analysis/utils/ess.py and sensititvity.py, the way make_golden_boot.py does) and
records what calc_log_mvnormal_pzs, calc_importance_weights, calc_ESS and filter_iqr return, the last two composed as gen_ess_bg of
mdqm9/analysis/results_00031.py composes them (that module imports rdkit and cannot be imported itself).

Inputs, per case: A atoms, 50 molecules, z ~ N(0, 1) float32 [50, A, 3], E1 ~ 5 N float64, neg_dlogp_bg and neg_dlogp_ti ~ 3 N
float32, from RandomState(7000 + A).  The reference gets the float32 arrays promoted to float64, so that it sums the stored values
themselves.  The case "A18_noti" has neg_dlogp_ti = 0 (a Boltzmann generator without a chained ambient map).

Asserted: every reference weight is finite and positive.  Guard of the filtered ESS (k = K_FILTER), recorded per case as ess_k_ok:
no weight lies within relative 1e-9 of a bound of filter_iqr, so the kept set does not depend on rounding; at least one case must
meet it.

Layout: names [C]; A [C]; per case c the rows off[c]:off[c+1] of E1, nd_bg, nd_ti, log_pz, w and z_flat[zoff[c]:zoff[c+1]]
([50, A, 3] row-major); ess [C] (k = None), ess_k [C], kept_k [C], ess_k_ok [C] at the filter multiple k."""
import argparse
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ATOMS = (1, 9, 18, 21, 22, 32)
N_MOL = 50
K_FILTER = 1.5
GUARD = 1e-9


def inputs(A, ti=True):
    rs = np.random.RandomState(7000 + A)
    z = rs.standard_normal((N_MOL, A, 3)).astype(np.float32)
    E1 = 5.0 * rs.standard_normal(N_MOL)
    nb = (3.0 * rs.standard_normal(N_MOL)).astype(np.float32)
    nt = (3.0 * rs.standard_normal(N_MOL)).astype(np.float32)
    return z, E1, nb, nt if ti else np.zeros(N_MOL, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TI_REFERENCE"), required=os.environ.get("TI_REFERENCE") is None)
    ap.add_argument("--out", default=os.path.join(HERE, "bg_reference.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    ess = importlib.import_module("mdqm9.analysis.utils.ess")
    sens = importlib.import_module("mdqm9.analysis.utils.sensititvity")

    cases = [(f"A{A}", A, True) for A in ATOMS] + [("A18_noti", 18, False)]
    cols = {k: [] for k in ("z", "E1", "nd_bg", "nd_ti", "log_pz", "w")}
    per = {k: [] for k in ("ess", "ess_k", "kept_k", "ess_k_ok")}
    for name, A, ti in cases:
        z, E1, nb, nt = inputs(A, ti)
        log_pz = ess.calc_log_mvnormal_pzs(z.reshape(N_MOL, -1).astype(np.float64))
        w = ess.calc_importance_weights(z0s=z.astype(np.float64), E1s=E1, neg_dlogps_bg=nb.astype(np.float64), neg_dlogps_ti=nt.astype(np.float64))
        assert np.isfinite(w).all() and (w > 0).all(), name
        keep = sens.filter_iqr(w, k=K_FILTER)
        q75, q25 = np.percentile(w, [75, 25])
        bounds = (q25 - K_FILTER * (q75 - q25), q75 + K_FILTER * (q75 - q25))
        ok = all(not (np.abs(w - b) <= GUARD * np.maximum(np.abs(w), abs(b))).any() for b in bounds) and keep.sum() > 0
        for k, v in dict(z=z.reshape(-1), E1=E1, nd_bg=nb, nd_ti=nt, log_pz=log_pz, w=w).items():
            cols[k].append(v)
        per["ess"].append(ess.calc_ESS(w))
        per["ess_k"].append(ess.calc_ESS(w[keep]) if keep.sum() else np.nan)
        per["kept_k"].append(int(keep.sum()))
        per["ess_k_ok"].append(bool(ok))
    assert any(per["ess_k_ok"]), "no case meets the guard of the filtered ESS"
    C = len(cases)
    np.savez_compressed(
        args.out, names=np.array([c[0] for c in cases]), A=np.array([c[1] for c in cases], np.int64), off=np.arange(C + 1) * N_MOL,
        zoff=np.cumsum([0] + [N_MOL * 3 * c[1] for c in cases]), z_flat=np.concatenate(cols["z"]).astype(np.float32),
        E1=np.concatenate(cols["E1"]), nd_bg=np.concatenate(cols["nd_bg"]).astype(np.float32), nd_ti=np.concatenate(cols["nd_ti"]).astype(np.float32),
        log_pz=np.concatenate(cols["log_pz"]), w=np.concatenate(cols["w"]), ess=np.array(per["ess"]), ess_k=np.array(per["ess_k"]),
        kept_k=np.array(per["kept_k"], np.int64), ess_k_ok=np.array(per["ess_k_ok"]), k=np.float64(K_FILTER))
    print(f"{C} cases, {os.path.getsize(args.out)} bytes; ess {np.round(per['ess'], 3)}; kept at k = {K_FILTER}: {per['kept_k']}; guard {per['ess_k_ok']}")

    # the numpy restatement against what was just recorded: the two bounds of tests/test_bg_host.py
    sys.path.insert(0, os.path.dirname(HERE))
    import bg_numpy as bgn
    worst = [0.0, 0.0]
    for name, A, ti in cases:
        z, E1, nb, nt = inputs(A, ti)
        m = 3 * A
        lp, lw = bgn.bg_logw(z.reshape(N_MOL, m), E1, nb, nt)
        ref_lp = ess.calc_log_mvnormal_pzs(z.reshape(N_MOL, -1).astype(np.float64))
        ref_lw = np.log(ess.calc_importance_weights(z0s=z.astype(np.float64), E1s=E1, neg_dlogps_bg=nb.astype(np.float64), neg_dlogps_ti=nt.astype(np.float64)))
        worst[0] = max(worst[0], (np.abs(lp - ref_lp) / (m * 2.0 ** -50 * np.abs(ref_lp))).max())
        bar = 2.0 ** -24 * np.abs(ref_lw) + m * 2.0 ** -50 * (np.abs(E1) + np.abs(ref_lp) + np.abs(nb) + np.abs(nt))
        worst[1] = max(worst[1], (np.abs(lw.astype(np.float64) - ref_lw) / bar).max())
    print(f"restatement vs reference, worst error as a fraction of the bars: logpz {worst[0]:.3f}, logw {worst[1]:.3f}")


if __name__ == "__main__":
    main()
