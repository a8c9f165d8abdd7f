"""fp64 numpy restatement of TICA as include/ti_hip.h defines it (ti_obs_tica_moments, ti_obs_tica_fit, ti_obs_tica_transform), the
second LAPACK route that cross-checks it, and the deterministic synthetic trajectories the tests share."""
import numpy as np

EPS = 2.0 ** -53
WELLS = np.array([-2.0 * np.pi / 3.0, 0.0, 2.0 * np.pi / 3.0])


def encode(x, enc=True):
    """[n, d] float64 features of x [n, K] float32: interleaved (cos, sin) of every value, or the values themselves"""
    x = np.asarray(x, np.float32).astype(np.float64)
    if not enc:
        return x
    out = np.empty((x.shape[0], 2 * x.shape[1]))
    out[:, 0::2], out[:, 1::2] = np.cos(x), np.sin(x)
    return out


def pairs(traj_off, tau):
    """first frames i of the pairs (i, i + tau) inside one trajectory: trajectory-major, then i ascending"""
    traj_off = np.asarray(traj_off, np.int64)
    parts = [np.arange(a, b - tau) for a, b in zip(traj_off[:-1], traj_off[1:]) if b - a > tau]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def moments(x, traj_off, lags, enc=True):
    """(count [L] int64, sum [L, 2, d], cov [L, 3, d, d]) with cov = (Sxx, Syy, Sxy)"""
    f = encode(x, enc)
    d = f.shape[1]
    count, sm, cov = np.zeros(len(lags), np.int64), np.zeros((len(lags), 2, d)), np.zeros((len(lags), 3, d, d))
    for l, tau in enumerate(lags):
        i = pairs(traj_off, int(tau))
        X, Y = f[i], f[i + int(tau)]
        count[l] = len(i)
        sm[l, 0], sm[l, 1] = X.sum(axis=0), Y.sum(axis=0)
        cov[l, 0], cov[l, 1], cov[l, 2] = X.T @ X, Y.T @ Y, X.T @ Y
    return count, sm, cov


def moments_bound(x, traj_off, lags, enc=True, c=8):
    """Entrywise bounds (bsum [L, 2, d], bcov [L, 3, d, d]) on |device - ``moments``|: 2 (sum_pairs |x_a| |y_b|) (N + c) 2^-53, with
    y = 1 for the sums.

    Write u = 2^-53.  Either side forms N products and adds them, each in one or two roundings, in some fixed order: a sum of N
    terms that have each passed through at most N roundings, so |error| <= N u sum |x_a| |y_b| to first order, whatever the order
    (Higham, Accuracy and Stability, 3.1); two sides: 2 N u.  The features: the cast of the fp32 value to fp64 is exact on both
    sides; with encode the device's sincos is within 2 ulp = 4 u relative and numpy's libm within 1 ulp = 2 u, so the two sides'
    features differ by at most 6 u relative and a product of two of them by 12 u = 2 * 6 u.  That is c = 6; c = 8 leaves room for the
    second-order terms (N u is below 1e-11 for every N the feature table admits).  Without encode c could be 0; the same c is used."""
    f = np.abs(encode(x, enc))
    d = f.shape[1]
    bsum, bcov = np.zeros((len(lags), 2, d)), np.zeros((len(lags), 3, d, d))
    for l, tau in enumerate(lags):
        i = pairs(traj_off, int(tau))
        X, Y = f[i], f[i + int(tau)]
        k = 2.0 * (len(i) + c) * EPS
        bsum[l, 0], bsum[l, 1] = k * X.sum(axis=0), k * Y.sum(axis=0)
        bcov[l, 0], bcov[l, 1], bcov[l, 2] = k * (X.T @ X), k * (Y.T @ Y), k * (X.T @ Y)
    return bsum, bcov


def covariances(count, sm, cov):
    """(mu, C00, C0t) of one lag"""
    n2 = 2.0 * float(count)
    mu = (sm[0] + sm[1]) / n2
    return mu, (cov[0] + cov[1]) / n2 - np.outer(mu, mu), (cov[2] + cov[2].T) / n2 - np.outer(mu, mu)


def fix_sign(R):
    """each column's entry of largest magnitude made positive; among exactly equal magnitudes the lowest index decides"""
    R = R.copy()
    for k in range(R.shape[1]):
        if np.all(np.isfinite(R[:, k])):
            f = int(np.argmax(np.abs(R[:, k])))            # argmax returns the first of equal maxima
            if R[f, k] < 0:
                R[:, k] = -R[:, k]
    return R


def fit(count, sm, cov, dim, epsilon=1e-6, scaling=True):
    """(mean [d], ev [dim], comp [d, dim], rank) of one lag by the whitening route of include/ti_hip.h"""
    mu, C00, C0t = covariances(count, sm, cov)
    d = len(mu)
    s, V = np.linalg.eigh(C00)
    s, V = s[::-1], V[:, ::-1]
    r = int((s > epsilon).sum())
    ev, comp = np.full(dim, np.nan), np.full((d, dim), np.nan)
    if r > 0:
        L = V[:, :r] / np.sqrt(s[:r])
        Kt = L.T @ C0t @ L
        lam, U = np.linalg.eigh(np.triu(Kt) + np.triu(Kt, 1).T)
        lam, U = lam[::-1], U[:, ::-1]
        nk = min(dim, r)
        ev[:nk] = lam[:nk]
        comp[:, :nk] = fix_sign(L @ U[:, :nk])
        if scaling:
            comp[:, :nk] = comp[:, :nk] * lam[:nk]
    return mu, ev, comp, r


def fit_generalized(count, sm, cov, dim, scaling=True):
    """The second route, full rank only: scipy.linalg.eigh(C0t, C00), whose eigenvectors W satisfy W^T C00 W = I as R does"""
    import scipy.linalg
    mu, C00, C0t = covariances(count, sm, cov)
    lam, W = scipy.linalg.eigh(C0t, C00)
    lam, W = lam[::-1][:dim], fix_sign(W[:, ::-1][:, :dim])
    return mu, lam, (W * lam if scaling else W), len(mu)


def transform(x, mean, comp, enc=True):
    """[B, dim] float64: (phi(x) - mu) R; a row with a non-finite value is NaN"""
    xf = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        y = (encode(np.where(np.isfinite(xf), xf, 0.0), enc) - mean) @ comp
    y[~np.all(np.isfinite(xf), axis=1)] = np.nan
    return y


def transform_bound(x, mean, comp, enc=True):
    """[B, dim]: the fp64 part of |device - ``transform``|: 2 (d + 8) 2^-53 sum_f (|phi_f| + |mu_f|) |R_fk|, as ``moments_bound`` (a
    subtraction and a product per term, d terms, the 6 u of the two sincos)"""
    f = np.abs(encode(np.where(np.isfinite(np.asarray(x, np.float32)), x, 0.0), enc)) + np.abs(mean)
    return 2.0 * (f.shape[1] + 8) * EPS * (f @ np.abs(np.nan_to_num(comp)))


def synthetic(K, lengths, seed=0):
    """(x [n, K] float32, traj_off [n_traj + 1] int64, wells [n, K] int8): column k sits in one of three wells (WELLS) on a line and
    steps to a neighbouring well with probability 0.002 * 3^k per frame, capped at 0.4 (a step off either end is not taken); 0.3 rad
    of Gaussian jitter about the well, wrapped to (-pi, pi].  Every trajectory starts in wells drawn afresh.  Deterministic in
    (K, lengths, seed)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(lengths)])
    n = int(off[-1])
    rate = np.minimum(0.002 * 3.0 ** np.arange(K), 0.4)
    hop = rng.random((n, K)) < rate
    step = np.where(rng.random((n, K)) < 0.5, -1, 1)
    start = rng.integers(0, 3, (len(lengths), K))
    wells = np.empty((n, K), np.int8)
    starts = set(off[:-1].tolist())
    s, t = None, 0
    for i in range(n):
        if i in starts:
            s, t = start[t].copy(), t + 1
        else:
            prop = s + step[i]
            s = np.where(hop[i] & (prop >= 0) & (prop <= 2), prop, s)
        wells[i] = s
    x = WELLS[wells] + 0.3 * rng.standard_normal((n, K))
    x = np.pi - np.mod(np.pi - x, 2.0 * np.pi)                   # (-pi, pi]
    return x.astype(np.float32), off, wells
