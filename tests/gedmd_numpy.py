"""fp64 numpy restatement of ti_obs_rff_gram (include/ti_hip.h) and of the host algebra behind observables.gedmd_spectrum: the
feature table, the Gram matrix as an ordinary matmul, the draws (tests/boot_numpy.py) and the spectrum through eigh of the Gram
matrix.  Written from the header's definitions; it is the oracle of the GPU tests and, with svd_route -- the reference's own
algorithm (an SVD of the m x p feature matrix per resample) restated -- the CPU side of tools/gedmd_bench.py."""
import numpy as np

import boot_numpy as bn

EPS = 2.0 ** -53


def pad(p):
    return -(-p // 16) * 16


def features(x, omega):
    """(c, s) [n, p] of x [n, d] fp32 and omega [d, p]: theta = x omega in fp64"""
    x = np.asarray(x, np.float32).astype(np.float64)
    theta = x.reshape(x.shape[0], -1) @ np.asarray(omega, np.float64)
    return np.cos(theta), np.sin(theta)


def weights(logw):
    logw = np.asarray(logw, np.float32).astype(np.float64)
    return np.exp(logw - logw.max())


def gram(x, omega, row=None, logw=None):
    """G [p, p] complex128 = M^H diag(w) M over the samples `row` (None: all, in order), M = c - i s"""
    c, s = features(x, omega)
    w = weights(logw) if logw is not None else np.ones(c.shape[0])
    if row is not None:
        c, s, w = c[row], s[row], w[row]
    M = c - 1j * s
    return (M.conj().T * w) @ M


def gram_rows(x, omega, logw=None, n_boot=0, seed=0, first=0, indices=None, n_draw=0):
    """[1 + n_boot, p, p]: the point estimate and the resamples, as ti_obs_rff_gram lays them out"""
    n = np.asarray(x).shape[0]
    rows = indices if indices is not None else bn.draw_rows(seed, first, n_boot, n_draw or n, n)
    return np.stack([gram(x, omega, None, logw)] + [gram(x, omega, r, logw) for r in rows])


def gram_bound(x, omega, row=None, logw=None):
    """2 W (4 n_draw + 2 (d + 1) Phi + 8) 2^-53: W the sum of the row's weights, Phi = max_n sum_i |x_i| max_k |omega_ik|"""
    x = np.asarray(x, np.float32).astype(np.float64)
    x = x.reshape(x.shape[0], -1)
    w = weights(logw) if logw is not None else np.ones(x.shape[0])
    nd = x.shape[0] if row is None else len(row)
    W = w.sum() if row is None else w[row].sum()
    phi = (np.abs(x) @ np.abs(np.asarray(omega, np.float64)).max(axis=1)).max()
    return 2 * W * (4 * nd + 2 * (x.shape[1] + 1) * phi + 8) * EPS


def spectrum(G, omega, a, nev, tol=0.0):
    """(d [nev] ascending, W [p, nev], r) of one Gram matrix: the reversible generator EDMD of the reference from G = M^H M"""
    omega = np.asarray(omega, np.float64)
    lam, U = np.linalg.eigh(G)
    lam, U = lam[::-1], U[:, ::-1]
    s = np.sqrt(np.maximum(lam, 0.0))
    r = max(int((s / s[0] >= tol).sum()), nev)
    L = U[:, :r] / s[:r]
    R = L.conj().T @ (-0.5 * a * (omega.T @ omega) * G) @ L
    d, Wi = np.linalg.eigh(0.5 * (R + R.conj().T))
    return d[-nev:], L @ Wi[:, -nev:], r


def svd_route(x, omega, a, nev, tol=0.0):
    """The reference's route restated (spectral_analysis_rff_generator, reversible): SVD of M^H [p, m]; (d, r)"""
    c, s = features(x, omega)
    M = c - 1j * s
    omega = np.asarray(omega, np.float64)
    ML = -0.5 * a * (omega.T @ omega) * (M.conj().T @ M)
    U, sv, _ = np.linalg.svd(M.conj().T, full_matrices=False)
    r = max(int((sv / sv[0] >= tol).sum()), nev)
    L = U[:, :r] / sv[:r]
    d = np.linalg.eigvalsh(L.conj().T @ ML @ L)
    return d[-nev:], r
