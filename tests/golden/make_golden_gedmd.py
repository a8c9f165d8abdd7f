#!/usr/bin/env python
"""Generate tests/golden/gedmd_reference.npz: the reference's reversible generator EDMD on random Fourier features, on seeded inputs.

    python tests/golden/make_golden_gedmd.py --reference /path/to/thermodynamic-interpolation

Only imports gedmd.rff.spectral_analysis_rff_generator from the reference checkout (numpy 2 has no np.infty, which gedmd/util.py names
in a default argument: it is set before the import) and records what it returns, called as adw/analysis/reweight_gedmd.py calls it
(a = 2 / beta, reversible=True, tol = the SVD cutoff), on the whole sample (the identity row) and on index rows of
np.random.RandomState(seed).choice(m, m), as bootstrap_eigenvalues draws them.

Samples: bimodal, coordinate 0 = +-1 + 0.35 N(0, 1), the others N(0, 1); Omega = RandomState(seed).randn(d, p) / sigma.

Guards (asserted per row; a seed that misses is skipped, the next one is tried, the seeds used and skipped are recorded):
  no singular ratio s / s_0 lies within 10 % of tol, so the rank does not depend on rounding;
  s[nev - 1] / s_0 >= tol, so the rmin branch (which divides by near-zero singular values) does not bind.

Also stored: ev_dev, the worst absolute eigenvalue difference between tests/gedmd_numpy.py (eigh of the Gram matrix) and the reference
(SVD of the feature matrix) over the fixture, on the machine that wrote it.

Layout: per case c x_flat[x_off[c]:x_off[c+1]] (fp32, [m, d]), omega_flat[om_off[c]:om_off[c+1]] ([d, p]), idx_flat[idx_off[c]:idx_off[c+1]]
(uint16, [3, m]), ev [n_case, 4 rows, 4] (NaN beyond nev; row 0 the identity row), rank [n_case, 4]."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gedmd_numpy as gn  # noqa: E402

CASES = ((1, 50, 4097, 4), (1, 50, 1000, 4), (1, 16, 257, 4), (2, 24, 1000, 4), (3, 17, 600, 3), (16, 32, 2000, 4), (1, 8, 65, 2))
SIGMA, BETA, TOL, N_ROWS = 0.6, 1.25, 1e-4, 3


class GuardMiss(Exception):
    pass


def make_case(ref, d, p, m, nev, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((m, d))
    x[:, 0] = np.where(rs.random_sample(m) < 0.5, -1.0, 1.0) + 0.35 * x[:, 0]
    x = x.astype(np.float32)
    omega = rs.randn(d, p) / SIGMA
    rows = [np.arange(m)] + [rs.choice(m, m) for _ in range(N_ROWS)]
    a = 2.0 / BETA
    ev, rank, dev = np.full((1 + N_ROWS, 4), np.nan), np.zeros(1 + N_ROWS, np.int64), 0.0
    for i, row in enumerate(rows):
        X = x[row].astype(np.float64).T
        s = np.linalg.svd(np.exp(-1j * X.T @ omega).conj().T, compute_uv=False)
        ratio = s / s[0]
        if (np.abs(ratio / TOL - 1.0) < 0.1).any() or ratio[nev - 1] < TOL:
            raise GuardMiss
        dj, Wj, M = ref(X, omega, nev, a=a, tol=TOL, reversible=True)
        ev[i, :nev], rank[i] = np.real(dj), int((ratio >= TOL).sum())
        mine, _, r = gn.spectrum(gn.gram(x, omega, row), omega, a, nev, TOL)
        assert r == rank[i], (r, rank[i])
        dev = max(dev, np.abs(mine - ev[i, :nev]).max())
    return x, omega, np.stack(rows[1:]), ev, rank, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "gedmd_reference.npz"))
    args = ap.parse_args()
    if not hasattr(np, "infty"):
        np.infty = np.inf
    sys.path.insert(0, args.reference)
    from gedmd.rff import spectral_analysis_rff_generator as ref
    xs, oms, idxs, evs, ranks, used, skipped, ev_dev = [], [], [], [], [], [], [], 0.0
    for c, (d, p, m, nev) in enumerate(CASES):
        seed = 100 * c
        while True:
            try:
                x, omega, idx, ev, rank, dev = make_case(ref, d, p, m, nev, seed)
                break
            except GuardMiss:
                skipped.append(seed)
                seed += 1
        used.append(seed)
        ev_dev = max(ev_dev, dev)
        xs.append(x.reshape(-1)); oms.append(omega.reshape(-1)); idxs.append(idx.astype(np.uint16).reshape(-1)); evs.append(ev); ranks.append(rank)
        print(f"case {c} (d, p, m, nev) = {(d, p, m, nev)}: seed {seed}, ranks {rank.tolist()}, dev {dev:.2e}")
    off = lambda parts: np.concatenate([[0], np.cumsum([a.size for a in parts])]).astype(np.int64)
    np.savez_compressed(args.out, cases=np.array(CASES, np.int64), x_flat=np.concatenate(xs), x_off=off(xs), omega_flat=np.concatenate(oms), om_off=off(oms),
                        idx_flat=np.concatenate(idxs), idx_off=off(idxs), ev=np.stack(evs), rank=np.stack(ranks), a=np.float64(2.0 / BETA),
                        tol=np.float64(TOL), sigma=np.float64(SIGMA), seeds=np.array(used, np.int64), skipped=np.array(skipped, np.int64),
                        ev_dev=np.float64(ev_dev))
    print(f"ev_dev {ev_dev:.3e}; skipped seeds {skipped}; {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
