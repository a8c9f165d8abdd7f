"""fp64 numpy restatement of ti_obs_eigh_wide and ti_obs_gedmd_spectrum_wide (include/ti_hip.h), written from the header's definitions:
the blocked two-sided Jacobi iteration over 32-wide index blocks in the round-robin ordering of tests/eigh_numpy.py, ONE sweep of that
module's cyclic Jacobi on the <= 64 indices of a block pair per visit with the whole matrix's threshold, every pair of a round formed
from the matrix as it stands at the start of the round.  The products are numpy's, so the restatement agrees with the device to
rounding, not bit for bit.  It is the oracle of tests/test_eigh_wide_host.py; the GPU tests print its sweep counts beside the device's."""
import numpy as np

import eigh_numpy as EN

EPS = EN.EPS
BLOCK, MAX_N, MAX_SWEEPS = 32, 1024, 64
SIZES = (65, 66, 96, 97, 129)
# outer sweeps of `eigh` on eigh_numpy.make(kind, n) for the kinds of eigh_numpy.KINDS in order: recorded once so that the GPU tests can
# print them beside the device's without running the restatement again; tests/test_eigh_wide_host.py holds them against `eigh`
SWEEPS = {65: (8, 17, 1, 15, 4), 66: (8, 19, 1, 16, 4), 96: (9, 21, 1, 18, 6), 97: (8, 19, 1, 17, 5), 129: (9, 23, 1, 20, 5)}


def launch_max(n):
    """Matrices per launch at order n: min(512, 2^31 / (32 n^2))"""
    return min(512, (1 << 31) // (32 * n * n))


def inner_sweep(S, thr):
    """One sweep of eigh_numpy.eigh's iteration on S [k, k] (in place) with the threshold thr: (U [k, k], rotated)"""
    n = S.shape[0]
    m = n + (n & 1)
    U = np.eye(n, dtype=np.complex128)
    rotated = False
    for r in range(m - 1):
        p, q = EN.round_pairs(m, r)
        keep = q < n
        p, q = p[keep], q[keep]
        b = S[p, q]
        ab = np.hypot(b.real, b.imag)
        rot = ab > thr
        if not rot.any():
            continue
        rotated = True
        p, q, b, ab = p[rot], q[rot], b[rot], ab[rot]
        tau = (S[q, q].real - S[p, p].real) / (2.0 * ab)
        t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
        c = 1.0 / np.sqrt(1.0 + t * t)
        s = t * c
        e = (b.real - 1j * b.imag) / ab
        se, ce = s * e, c * e
        for M in (S, U):
            xp, xq = M[:, p].copy(), M[:, q].copy()
            M[:, p] = c * xp - se * xq
            M[:, q] = s * xp + ce * xq
        xp, xq = S[p, :].copy(), S[q, :].copy()
        S[p, :] = c[:, None] * xp - se.conj()[:, None] * xq
        S[q, :] = s[:, None] * xp + ce.conj()[:, None] * xq
        S[p, q] = 0.0
        S[q, p] = 0.0
        S[p, p] = S[p, p].real
        S[q, q] = S[q, q].real
    return U, rotated


def eigh(a, stats=None):
    """(w [n] ascending, v [n, n], outer sweeps) of one matrix a [n, n]; n <= 64 is eigh_numpy.eigh.  stats (a dict) receives the
    count of inner sweeps that rotated."""
    A = EN.hermitian_from_upper(a)
    n = A.shape[0]
    if n <= EN.MAX_N:
        return EN.eigh(a)
    if n > MAX_N:
        raise ValueError(f"n must be in 1..{MAX_N}")
    if not np.isfinite(A).all():
        raise FloatingPointError("non-finite entry")
    thr = EPS * np.abs(np.diag(A).real).max()
    nb = -(-n // BLOCK)
    mb = nb + (nb & 1)
    V = np.eye(n, dtype=np.complex128)
    sweeps = inner = 0
    while True:
        sweeps += 1
        if sweeps > MAX_SWEEPS:
            raise ArithmeticError(f"still rotating after {MAX_SWEEPS} sweeps")
        rotated = False
        for r in range(mb - 1):
            I, J = EN.round_pairs(mb, r)
            visits = []
            for bi, bj in zip(I, J):
                if bj >= nb:                               # the pad block
                    continue
                idx = np.r_[bi * BLOCK:(bi + 1) * BLOCK, bj * BLOCK:min((bj + 1) * BLOCK, n)]
                S = A[np.ix_(idx, idx)].copy()             # every pair from the matrix at the start of the round
                U, rot = inner_sweep(S, thr)
                if rot:
                    visits.append((idx, U, S))
            rotated = rotated or bool(visits)
            inner += len(visits)
            for idx, U, S in visits:                       # columns of A and V
                A[:, idx] = A[:, idx] @ U
                V[:, idx] = V[:, idx] @ U
            for idx, U, S in visits:                       # rows of A, then the swept block
                A[idx, :] = U.conj().T @ A[idx, :]
            for idx, U, S in visits:
                A[np.ix_(idx, idx)] = S
        if not rotated:
            break
    if stats is not None:
        stats["inner"] = inner
    d = np.diag(A).real
    order = np.argsort(d, kind="stable")
    return d[order], V[:, order], sweeps


def spectrum(G, omega, a, nev, tol=0.0):
    """eigh_numpy.spectrum with the blocked solver for both solves: (d [nev] ascending, W [p, nev], r)"""
    omega = np.asarray(omega, np.float64)
    G = EN.hermitian_from_upper(G)
    lam, U, _ = eigh(G)
    lam, U = lam[::-1], U[:, ::-1]
    s = np.sqrt(np.maximum(lam, 0.0))
    r = max(int((s / s[0] >= tol).sum()), nev)
    L = U[:, :r] / s[:r]
    R = L.conj().T @ ((-0.5 * a) * (omega.T @ omega) * G) @ L
    d, Wi, _ = eigh(0.5 * (R + R.conj().T))
    return d[-nev:], L @ Wi[:, -nev:], r
