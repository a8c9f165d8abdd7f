"""fp64 numpy restatement of ti_obs_eigh and ti_obs_gedmd_spectrum (include/ti_hip.h), written from the header's definitions: the
parallel cyclic two-sided Jacobi iteration in the round-robin ordering, every rotation of a round computed from the matrix as it
stands at the start of the round, and the spectrum algebra of tests/gedmd_numpy.py with that solver in place of LAPACK's.  It is the
oracle of tests/test_eigh_host.py and of the GPU tests; `cases` builds the 45 matrices both compare against numpy.linalg.eigh."""
import numpy as np

EPS = 2.0 ** -53
MAX_N, MAX_SWEEPS = 64, 64
SIZES = (1, 2, 3, 15, 16, 17, 33, 63, 64)
KINDS = ("random", "gram", "identity", "degenerate", "rank1")


def round_pairs(m, r):
    """(p, q), p < q: the m / 2 disjoint pairs of round r of the tournament over m slots -- slot 0 holds index 0, slot k >= 1 holds
    index 1 + (k - 1 + r) mod (m - 1), slot i meets slot m - 1 - i"""
    k = np.arange(m)
    idx = np.where(k == 0, 0, 1 + (k - 1 + r) % (m - 1))
    a, b = idx[:m // 2], idx[::-1][:m // 2]
    return np.minimum(a, b), np.maximum(a, b)


def hermitian_from_upper(a):
    """The matrix ti_obs_eigh sees: the upper triangle, the real part of the diagonal, the conjugate below"""
    a = np.asarray(a, np.complex128)
    u = np.triu(a, 1)
    return u + u.conj().T + np.diag(np.diag(a).real)


def eigh(a):
    """(w [n] ascending, v [n, n], sweeps) of one matrix a [n, n]"""
    A = hermitian_from_upper(a)
    n = A.shape[0]
    if not 1 <= n <= MAX_N:
        raise ValueError(f"n must be in 1..{MAX_N}")
    if not np.isfinite(A).all():
        raise FloatingPointError("non-finite entry")
    m = n + (n & 1)
    thr = EPS * np.abs(np.diag(A).real).max()
    V = np.eye(n, dtype=np.complex128)
    sweeps = 0
    while True:
        sweeps += 1
        if sweeps > MAX_SWEEPS:
            raise ArithmeticError(f"still rotating after {MAX_SWEEPS} sweeps")
        rotated = False
        for r in range(m - 1):
            p, q = round_pairs(m, r)
            keep = q < n                                   # a pair with the pad index is skipped
            p, q = p[keep], q[keep]
            b = A[p, q]
            ab = np.hypot(b.real, b.imag)
            rot = ab > thr
            if not rot.any():
                continue
            rotated = True
            p, q, b, ab = p[rot], q[rot], b[rot], ab[rot]
            tau = (A[q, q].real - A[p, p].real) / (2.0 * ab)
            t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = t * c
            e = (b.real - 1j * b.imag) / ab
            se, ce = s * e, c * e
            for M in (A, V):                               # columns: M <- M U
                xp, xq = M[:, p].copy(), M[:, q].copy()
                M[:, p] = c * xp - se * xq
                M[:, q] = s * xp + ce * xq
            xp, xq = A[p, :].copy(), A[q, :].copy()        # rows: A <- U^H A
            A[p, :] = c[:, None] * xp - se.conj()[:, None] * xq
            A[q, :] = s[:, None] * xp + ce.conj()[:, None] * xq
            A[p, q] = 0.0
            A[q, p] = 0.0
            A[p, p] = A[p, p].real
            A[q, q] = A[q, q].real
        if not rotated:
            break
    d = np.diag(A).real
    order = np.argsort(d, kind="stable")                   # equal eigenvalues: by the diagonal position they converged at
    return d[order], V[:, order], sweeps


def eigh_batched(a):
    a = np.asarray(a, np.complex128)
    out = [eigh(x) for x in a]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32)


def spectrum(G, omega, a, nev, tol=0.0):
    """tests/gedmd_numpy.spectrum with the Jacobi solver: (d [nev] ascending, W [p, nev], r)"""
    omega = np.asarray(omega, np.float64)
    G = hermitian_from_upper(G)
    lam, U, _ = eigh(G)
    lam, U = lam[::-1], U[:, ::-1]
    s = np.sqrt(np.maximum(lam, 0.0))
    r = max(int((s / s[0] >= tol).sum()), nev)
    L = U[:, :r] / s[:r]
    R = L.conj().T @ ((-0.5 * a) * (omega.T @ omega) * G) @ L
    d, Wi, _ = eigh(0.5 * (R + R.conj().T))
    return d[-nev:], L @ Wi[:, -nev:], r


def _unitary(rs, n):
    q, _ = np.linalg.qr(rs.standard_normal((n, n)) + 1j * rs.standard_normal((n, n)))
    return q


def make(kind, n, seed=0):
    """One test matrix [n, n] complex128, exactly Hermitian"""
    rs = np.random.RandomState(1000 * KINDS.index(kind) + n + 100000 * seed)
    if kind == "random":
        x = rs.standard_normal((n, n)) + 1j * rs.standard_normal((n, n))
        return hermitian_from_upper(x + x.conj().T)
    if kind == "identity":
        return 3.0 * np.eye(n, dtype=np.complex128)
    if kind == "rank1":
        v = rs.standard_normal(n) + 1j * rs.standard_normal(n)
        return hermitian_from_upper(np.outer(v, v.conj()))
    if kind == "gram":                                     # Gram-like: PSD, numerically rank-deficient
        lam = 4096.0 * 10.0 ** (-20.0 * np.arange(n) / max(n - 1, 1))
    else:                                                  # four-fold degenerate spectrum
        lam = np.array([5.0, 2.0, 2.0, -1.0])[np.arange(n) % 4]
    q = _unitary(rs, n)
    return hermitian_from_upper((q * lam) @ q.conj().T)


def cases():
    """[(name, matrix)] of the 45 matrices: SIZES x KINDS"""
    return [(f"{kind}-n{n}", make(kind, n)) for n in SIZES for kind in KINDS]


def errors(A, w, v):
    """(eigenvalue error, residual, orthogonality defect) of a result against numpy.linalg.eigh(A, UPLO="U"): the first two in units
    of n eps ||A||_F, the third in units of n eps"""
    A = hermitian_from_upper(A)
    n = A.shape[0]
    unit = n * EPS * np.linalg.norm(A)
    ref = np.linalg.eigh(A, UPLO="U")[0]
    ev = np.abs(w - ref).max() / unit
    res = np.abs(A @ v - v * w).max() / unit
    orth = np.abs(v.conj().T @ v - np.eye(n)).max() / (n * EPS)
    return ev, res, orth
