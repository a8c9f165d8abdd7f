"""fp64 numpy restatement of ti_obs_bootstrap (include/ti_hip.h): the Philox draws, the IQR filter, the three estimators, the three
filter modes and the percentile interval.  Written from the header's definitions; it is the oracle of the generator's draws and the
CPU side of tools/boot_bench.py."""
import numpy as np

ESS, TFEP, MEAN = 0, 1, 2
NONE, ONCE, RESAMPLE = 0, 1, 2
DOMAIN = 0x424F4F54
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint64 arrays holding 32-bit values) of Philox4x32-10 on counters c0..c3 (broadcastable) with key (k0, k1)."""
    c = [np.asarray(v, np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def draws(seed, R, n_draw, n_pop):
    """The n_draw population indices (int32) of global resample R: draw j = (u * n_pop) >> 64, u = o[2 (j & 1)] | o[2 (j & 1) + 1] << 32
    of o = Philox4x32-10((j >> 1, R lo, R hi, DOMAIN), key = (seed lo, seed hi))."""
    seed, R = int(seed) & (2**64 - 1), int(R) & (2**64 - 1)
    pairs = np.arange((n_draw + 1) // 2, dtype=np.uint64)
    o = philox4x32_10(pairs, R & 0xFFFFFFFF, R >> 32, DOMAIN, seed & 0xFFFFFFFF, seed >> 32)
    lo = np.stack([o[0], o[2]], axis=1).reshape(-1)[:n_draw]
    hi = np.stack([o[1], o[3]], axis=1).reshape(-1)[:n_draw]
    n = np.uint64(n_pop)                              # n_pop < 2^31: hi * n + (lo * n >> 32) < 2^64
    return ((hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)).astype(np.int32)


def draw_rows(seed, first, n_boot, n_draw, n_pop):
    return np.stack([draws(seed, first + r, n_draw, n_pop) for r in range(n_boot)]) if n_boot else np.zeros((0, n_draw), np.int32)


def percentile(x, p):
    """numpy's default rule at fraction p of the values x: linear between the neighbours of position (len - 1) p."""
    s = np.sort(np.asarray(x, np.float64))
    pos = (s.size - 1) * p
    i = int(np.floor(pos))
    return s[i] if i + 1 >= s.size else s[i] + (pos - i) * (s[i + 1] - s[i])


def keep_mask(x, k):
    q25, q75 = percentile(x, 0.25), percentile(x, 0.75)
    iqr = q75 - q25
    return (x > q25 - k * iqr) & (x < q75 + k * iqr)


def estimate(v, m, estimator, k=None):
    """(estimate, kept count) over the multiset of fp32 values v (shift m), filtered by its own quartiles when k is given."""
    v = np.asarray(v, np.float64)
    w = np.exp(v - m)
    if k is not None:
        keep = keep_mask(v if estimator == MEAN else w, k)
        v, w = v[keep], w[keep]
    if v.size == 0:
        return np.nan, 0
    if estimator == ESS:
        return w.sum() ** 2 / (w * w).sum(), v.size
    if estimator == TFEP:
        return -(m + np.log(w.sum() / v.size)), v.size
    return -(v.sum() / v.size), v.size


def bootstrap(logw, estimator, filter=NONE, k=1.0, level=0.95, n_boot=1000, first=0, seed=0, indices=None, n_draw=0):
    """(point, lower, upper, kept, estimates [n_boot]) as ti_obs_bootstrap defines them."""
    logw = np.asarray(logw, np.float32)
    m = float(logw.max())
    kk = None if filter == NONE else k
    point, kept = estimate(logw, m, estimator, kk)
    pop = logw
    if filter == ONCE:
        w = np.exp(logw.astype(np.float64) - m)
        pop = logw[keep_mask(logw.astype(np.float64) if estimator == MEAN else w, k)]
    nd = indices.shape[1] if indices is not None else (n_draw or pop.size)
    est = np.full(n_boot, np.nan)
    for r in range(n_boot if pop.size else 0):
        ix = indices[r] if indices is not None else draws(seed, first + r, nd, pop.size)
        est[r] = estimate(pop[ix], m, estimator, k if filter == RESAMPLE else None)[0]
    if n_boot == 0 or np.isnan(est).any():
        return point, np.nan, np.nan, kept, est
    return point, percentile(est, (1 - level) / 2), percentile(est, (1 + level) / 2), kept, est


def reference_loop(logw, estimator, filter=NONE, k=1.0, n_boot=1000, rs=None):
    """The reference's loop (results_00031.py gen_*) with its own tools -- RandomState.choice for the draws, np.percentile inside the
    filter -- on phi = -logw in fp64: (point, lower, upper, estimates).  The CPU side of tools/boot_bench.py."""
    rs = rs or np.random.RandomState(0)
    phis = -np.asarray(logw, np.float64)

    def mask(p):
        x = p if estimator == MEAN else np.exp(-p)
        q75, q25 = np.percentile(x, [75, 25])
        return (x > q25 - k * (q75 - q25)) & (x < q75 + k * (q75 - q25))

    def est_of(p):
        if p.size == 0:
            return np.nan
        if estimator == ESS:
            w = np.exp(-p)
            return np.square(w.sum()) / np.square(w).sum()
        return p.mean() if estimator == MEAN else -np.log(np.exp(-p).sum() / p.size)

    kept = phis if filter == NONE else phis[mask(phis)]
    pop = kept if filter == ONCE else phis
    est = np.zeros(n_boot)
    for i in range(n_boot):
        p = pop[rs.choice(np.arange(len(kept)), len(kept), replace=True)]
        est[i] = est_of(p[mask(p)] if filter == RESAMPLE else p)
    lo, hi = np.percentile(est, [2.5, 97.5]) if n_boot else (np.nan, np.nan)
    return est_of(kept), lo, hi, est
