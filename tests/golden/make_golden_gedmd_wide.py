#!/usr/bin/env python
"""Generate tests/golden/gedmd_wide_reference.npz: the reference's reversible generator EDMD and its cross-validated VAMP score at the
molecule study's sizes (p up to 513), on seeded inputs.

    python tests/golden/make_golden_gedmd_wide.py --reference /path/to/thermodynamic-interpolation

Imports gedmd.rff.spectral_analysis_rff_generator and cv_generator_rff from the reference checkout (np.infty is set first, as in
make_golden_gedmd.py; sklearn and scipy are needed) and records what they return.  gedmd.rff.train_test_split is replaced in memory by
a function that permutes with a seeded RandomState, records the permutation and cuts it at floor(train_size * m), sklearn's sizes.

Samples as in make_golden_gedmd.py (bimodal coordinate 0, the others N(0, 1)); the torsion-like cases (wrap = 1) are scaled by 1.5 and
wrapped to (-pi, pi].  Omega = RandomState(seed).randn(d, p) / sigma.  Per case: the whole sample and three RandomState.choice(m, m) rows
through spectral_analysis_rff_generator, and three recorded 75 / 25 splits through cv_generator_rff.

Guard (every stored row and every training set; a seed that misses is skipped, the next is tried, both lists are recorded): only the
cut is guarded -- s_r / s_0 >= tol (1 + 1e-3) and s_{r+1} / s_0 <= tol (1 - 1e-3), r the rank -- and s[nev - 1] / s_0 >= tol, so the rmin
branch does not bind.  (With hundreds of singular values crossing four decades some ratio always lies close to tol; only the two at
the cut decide the rank.)

Also stored: ev_dev and score_dev, the worst absolute difference between the Gram-only restatement (tests/gedmd_numpy.py,
tests/gedmd_wide_numpy.py) and the reference over the fixture, on the machine that wrote it.

Layout: cases [n_case, 5] = (d, p, m, nev, wrap), sigma [n_case], a [n_case]; per case c x_flat[x_off[c]:x_off[c+1]] (fp32, [m, d]),
omega_flat[om_off[c]:om_off[c+1]] ([d, p]), idx_flat[idx_off[c]:idx_off[c+1]] (uint16, [3, m]: the choice rows), perm_flat likewise
(uint16, [3, m]: the splits); ev [n_case, 4, 4] and rank [n_case, 4] (row 0 the whole sample), cv_ev [n_case, 3, 4], cv_score [n_case, 3],
cv_rank [n_case, 3]; NaN beyond nev."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gedmd_numpy as gn  # noqa: E402
import gedmd_wide_numpy as gw  # noqa: E402

# (d, p, m, nev, wrap, sigma, a): a = k_B T at 300 K for the torsion-like cases, 2 / beta of make_golden_gedmd.py for the rest
KT, A0 = 0.008314462618 * 300.0, 2.0 / 1.25
CASES = ((6, 300, 3000, 4, 1, 5.0, KT), (6, 300, 3000, 4, 1, 2.0, KT), (2, 130, 1500, 4, 0, 0.6, A0), (1, 50, 1000, 4, 0, 0.6, A0),
         (1, 16, 257, 4, 0, 0.6, A0), (6, 513, 2000, 4, 1, 2.0, KT))
TOL, RTRAIN, N_ROWS, N_SPLIT, MARGIN = 1e-4, 0.75, 3, 3, 1e-3


class GuardMiss(Exception):
    pass


def guarded_rank(x, omega, nev):
    s = np.linalg.svd(np.exp(-1j * x.astype(np.float64) @ omega).conj().T, compute_uv=False)
    ratio = s / s[0]
    r = int((ratio >= TOL).sum())
    if ratio[r - 1] < TOL * (1 + MARGIN) or (r < len(s) and ratio[r] > TOL * (1 - MARGIN)) or ratio[nev - 1] < TOL:
        raise GuardMiss
    return r


def make_case(rff, d, p, m, nev, wrap, sigma, a, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((m, d))
    x[:, 0] = np.where(rs.random_sample(m) < 0.5, -1.0, 1.0) + 0.35 * x[:, 0]
    if wrap:
        x = np.pi - np.mod(np.pi - 1.5 * x, 2 * np.pi)                       # (-pi, pi]
    x = x.astype(np.float32)
    omega = rs.randn(d, p) / sigma
    rows = [np.arange(m)] + [rs.choice(m, m) for _ in range(N_ROWS)]
    ev, rank, ev_dev = np.full((1 + N_ROWS, 4), np.nan), np.zeros(1 + N_ROWS, np.int64), 0.0
    for i, row in enumerate(rows):
        rank[i] = guarded_rank(x[row], omega, nev)
        dj, _, _ = rff.spectral_analysis_rff_generator(x[row].astype(np.float64).T, omega, nev, a=a, tol=TOL, reversible=True)
        ev[i, :nev] = np.real(dj)
        mine, _, r = gn.spectrum(gn.gram(x, omega, row), omega, a, nev, TOL)
        assert r == rank[i], (r, rank[i])
        ev_dev = max(ev_dev, np.abs(mine - ev[i, :nev]).max())
    # the splits: the reference draws them through train_test_split, replaced by a recording permutation
    perms, split_rs = [], np.random.RandomState(seed + 7919)

    def recording_split(X, train_size):
        perm = split_rs.permutation(X.shape[0])
        perms.append(perm)
        n_train = int(np.floor(train_size * X.shape[0]))
        return X[perm[:n_train]], X[perm[n_train:]]

    rff.train_test_split = recording_split
    dcv, score = rff.cv_generator_rff(x.astype(np.float64).T, omega, float(a), RTRAIN, N_SPLIT, nev, tol=TOL)
    n_train = int(np.floor(RTRAIN * m))
    cv_ev, cv_rank, score_dev = np.full((N_SPLIT, 4), np.nan), np.zeros(N_SPLIT, np.int64), 0.0
    for i, perm in enumerate(perms):
        cv_rank[i] = guarded_rank(x[perm[:n_train]], omega, nev)
        cv_ev[i, :nev] = np.real(dcv[i])
        mine, sc, r = gw.cv_split(x, omega, a, nev, TOL, perm, n_train)
        assert r == cv_rank[i], (r, cv_rank[i])
        ev_dev = max(ev_dev, np.abs(mine - cv_ev[i, :nev]).max())
        score_dev = max(score_dev, abs(sc - score[i]))
    return x, omega, np.stack(rows[1:]), np.stack(perms), ev, rank, cv_ev, np.asarray(score), cv_rank, ev_dev, score_dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "gedmd_wide_reference.npz"))
    args = ap.parse_args()
    if not hasattr(np, "infty"):
        np.infty = np.inf
    sys.path.insert(0, args.reference)
    import gedmd.rff as rff
    keys = ("x", "omega", "idx", "perm", "ev", "rank", "cv_ev", "cv_score", "cv_rank")
    parts, used, skipped, ev_dev, score_dev = {k: [] for k in keys}, [], [], 0.0, 0.0
    for c, (d, p, m, nev, wrap, sigma, a) in enumerate(CASES):
        seed = 100 * c
        while True:
            try:
                res = make_case(rff, d, p, m, nev, wrap, sigma, a, seed)
                break
            except GuardMiss:
                skipped.append(seed)
                seed += 1
        used.append(seed)
        for k, v in zip(keys, res):
            parts[k].append(v)
        ev_dev, score_dev = max(ev_dev, res[-2]), max(score_dev, res[-1])
        print(f"case {c} (d, p, m, nev) = {(d, p, m, nev)} sigma {sigma}: seed {seed}, ranks {res[5].tolist()} cv {res[8].tolist()}, "
              f"ev dev {res[-2]:.2e}, score dev {res[-1]:.2e}", flush=True)
    off = lambda ps: np.concatenate([[0], np.cumsum([a.size for a in ps])]).astype(np.int64)
    flat = lambda ps, dt=None: np.concatenate([np.asarray(a, dt).reshape(-1) for a in ps])
    np.savez_compressed(
        args.out, cases=np.array([c[:5] for c in CASES], np.int64), sigma=np.array([c[5] for c in CASES]), a=np.array([c[6] for c in CASES]),
        x_flat=flat(parts["x"]), x_off=off(parts["x"]), omega_flat=flat(parts["omega"]), om_off=off(parts["omega"]),
        idx_flat=flat(parts["idx"], np.uint16), idx_off=off(parts["idx"]), perm_flat=flat(parts["perm"], np.uint16), perm_off=off(parts["perm"]),
        ev=np.stack(parts["ev"]), rank=np.stack(parts["rank"]), cv_ev=np.stack(parts["cv_ev"]), cv_score=np.stack(parts["cv_score"]),
        cv_rank=np.stack(parts["cv_rank"]), tol=np.float64(TOL), rtrain=np.float64(RTRAIN), seeds=np.array(used, np.int64),
        skipped=np.array(skipped, np.int64), ev_dev=np.float64(ev_dev), score_dev=np.float64(score_dev))
    print(f"ev_dev {ev_dev:.3e}; score_dev {score_dev:.3e}; skipped seeds {skipped}; {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
