"""fp64 numpy restatement of the cross-validated gEDMD score from Gram matrices alone (observables.gedmd_vamp_score / gedmd_cv), next to
tests/gedmd_numpy.py: the reference's gedmd/rff.py cv_generator_rff sees the feature matrices of the training and the held-out set;
this sees G_train and G_test.  Written from the definitions in the docstrings; matrix by matrix, no batching.  Also the tile
bookkeeping of the blocked Gram pass (csrc/obs_gram_kernels.hip obs_gram_wide_kernel), restated for the numbering test."""
import numpy as np

import gedmd_numpy as gn


def vamp_score(G_test, omega, a, W):
    """sum eig of L0^H ML_test L0 with L0 = W U0 / sqrt(lambda), (lambda, U0) = eigh(W^H G_test W); NaN unless every lambda > 0"""
    omega = np.asarray(omega, np.float64)
    C = W.conj().T @ G_test @ W
    lam, U0 = np.linalg.eigh(0.5 * (C + C.conj().T))
    if not (lam > 0).all():
        return np.nan
    L0 = (W @ U0) / np.sqrt(lam)
    R = L0.conj().T @ (-0.5 * a * (omega.T @ omega) * G_test) @ L0
    return float(np.linalg.eigvalsh(0.5 * (R + R.conj().T)).sum())


def cv_split(x, omega, a, nev, tol, perm, n_train, logw=None):
    """(d [nev], score, rank) of one split: perm[:n_train] trains, perm[n_train:] scores"""
    perm = np.asarray(perm, np.int64)
    d, W, r = gn.spectrum(gn.gram(x, omega, perm[:n_train], logw), omega, a, nev, tol)
    return d, vamp_score(gn.gram(x, omega, perm[n_train:], logw), omega, a, W), r


def wide_launch_tiles(T):
    """Every (k, l, slot) the blocked pass writes for T > 8 column tiles, launch by launch as launch_obs_gram_wide cuts them: k <= l
    the tile's row and column in the whole matrix, slot the partial-tile number it is stored at."""
    nf, tl = divmod(T, 8)
    shapes = [(8, True, 0, -1, nf)] + ([(tl, True, nf, -1, 1)] if tl else []) + ([(8, False, nf, -1, nf * (nf - 1) // 2)] if nf > 1 else []) \
        + ([(tl, False, nf, nf, nf)] if tl else [])
    out = []
    for tj, diag, pi0, jfix, cnt in shapes:
        ti = tj if diag else 8
        nt = tj * (tj + 1) // 2 if diag else ti * tj
        for c in range(cnt):
            if diag:
                pi = pj = pi0 + c
            elif jfix >= 0:
                pi, pj = c, jfix
            else:
                pi, rem = 0, c
                while rem >= pi0 - 1 - pi:
                    rem -= pi0 - 1 - pi
                    pi += 1
                pj = pi + 1 + rem
            for t in range(nt):
                if diag:
                    a = 0
                    while t >= tj - a:
                        t -= tj - a
                        a += 1
                    b = a + t
                else:
                    a, b = divmod(t, tj)
                k, l = 8 * pi + a, 8 * pj + b
                out.append((k, l, k * T - k * (k - 1) // 2 + (l - k)))
    return out
