"""fp64 numpy restatement of the velocity loss (include/ti_hip.h ti_painn_vloss / ti_adw_vloss): the interpolant with its three gamma
kinds, the centring modes, the per-molecule loss with the magnitudes its error bound needs, the time profile, and the Philox time
draws.  Shared by tests/test_vloss_host.py, tests/test_gpu_vloss.py and tests/golden/make_golden_vloss.py; states are [B, A, 3]
(molecules) or [B, d] / [B] (adw), times [B].  `a` is used as passed: the reference holds it as a float32 tensor, so float(np.float32(a)) reproduces it."""
import numpy as np

VLOSS_DOMAIN = 0x564C4F53
SIG_SCALE = float(np.float32(2.2))                          # the reference's torch.tensor(2.2)
T_MAX = np.float32(1.0) - np.float32(2.0 ** -24)          # the cap of a drawn t: the largest float32 below 1


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def gamma(kind, a, t):
    t = np.asarray(t, np.float64)
    if kind == "brownian":
        return np.sqrt(a * t * (1.0 - t))
    if kind == "sin2":
        return np.sin(np.pi * t) ** 2
    if kind == "sig_sum":
        return SIG_SCALE * (sigmoid(a * (t - 0.5) + 1.0) - sigmoid(a * (t - 0.5) - 1.0) - sigmoid(1.0 - a / 2) + sigmoid(-1.0 - a / 2))
    raise NotImplementedError(kind)


def gamma_dot(kind, a, t):
    t = np.asarray(t, np.float64)
    if kind == "brownian":
        with np.errstate(divide="ignore", invalid="ignore"):
            return a * (1.0 - 2.0 * t) / (2.0 * np.sqrt(a * t * (1.0 - t)))
    if kind == "sin2":
        return 2.0 * np.pi * np.sin(np.pi * t) * np.cos(np.pi * t)
    if kind == "sig_sum":
        sp, sm = sigmoid(a * (t - 0.5) + 1.0), sigmoid(a * (t - 0.5) - 1.0)
        return SIG_SCALE * a * ((1.0 - sp) * sp - (1.0 - sm) * sm)
    raise NotImplementedError(kind)


def _per_mol(t, x):
    """t [B] broadcast against a state array x [B, ...]"""
    return np.asarray(t, np.float64).reshape((-1,) + (1,) * (np.ndim(x) - 1))


def interpolate(x0, x1, t, z=None, *, kind="standard", gamma_kind="brownian", a=1.0, center="batch", return_abs=False):
    """-> (xt [2, ...] float64 (one_sided: [1, ...]), S [2, ...]): the centred states and the magnitude
    S = |(1 - t) x0| + |t x1| + |gamma z| + |mean| every error bound of stage one is stated in.  return_abs: also [halves, components]
    (adw in one dimension: [halves]), the sum over the rows of |raw| of the uncentred states, which bounds the rounding of a column sum."""
    x0, x1 = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    tt = _per_mol(t, x0)
    it = (1.0 - tt) * x0 + tt * x1
    mag = np.abs((1.0 - tt) * x0) + np.abs(tt * x1)
    if kind == "one_sided":
        xs, mags = [tt * x1 + (1.0 - tt) * x0], [mag]
    else:
        gz = gamma(gamma_kind, a, tt) * np.asarray(z, np.float64)
        xs, mags = [it + gz, it - gz], [mag + np.abs(gz)] * 2
    out, S = [], []
    for x, m in zip(xs, mags):
        if center == "batch":            # the mean over all atom rows of the call, per component
            mean = x.reshape(-1, x.shape[-1]).mean(axis=0) if x.ndim == 3 else x.mean(axis=0)
        elif center == "molecule":
            mean = x.mean(axis=1, keepdims=True)
        else:
            mean = 0.0
        out.append(x - mean)
        S.append(m + np.abs(mean))
    if return_abs:
        rows = lambda x: x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x
        return np.stack(out), np.stack(S), np.stack([np.abs(rows(x)).sum(axis=0) for x in xs])
    return np.stack(out), np.stack(S)


def loss(x0, x1, t, z, bp, bm=None, *, kind="standard", gamma_kind="brownian", a=1.0):
    """-> (l [B], sum of |terms| [B], n_terms): the per-molecule loss, with what its rounding bound n_terms 2^-53 sum|terms| needs."""
    x0, x1, bp = (np.asarray(v, np.float64) for v in (x0, x1, bp))
    B = x0.shape[0]
    d = x1 - x0
    if kind == "one_sided":
        terms = [0.5 * bp * bp, -d * bp]
    else:
        bm, gz = np.asarray(bm, np.float64), gamma_dot(gamma_kind, a, _per_mol(t, x0)) * np.asarray(z, np.float64)
        terms = [0.5 * bp * bp, -(d + gz) * bp, 0.5 * bm * bm, -(d - gz) * bm]
    flat = np.stack([v.reshape(B, -1) for v in terms], axis=-1).reshape(B, -1)          # element order, the terms of an element together
    return flat.sum(axis=1), np.abs(flat).sum(axis=1), flat.shape[1]


def row_loss(x0, x1, t, z, bp, bm=None, **kw):
    """The reference's vmapped loss: one value per atom row [B A] of molecules [B, A, 3]"""
    f = lambda v: None if v is None else np.asarray(v, np.float64).reshape(-1, 3)
    A = np.shape(x0)[1]
    return loss(f(x0), f(x1), np.repeat(np.asarray(t, np.float64), A), f(z), f(bp), f(bm), **kw)[0]


def time_bins(l, t, n):
    """[n, 2]: the sum of l and the count per equal-width bin of t on [0, 1], t = 1 in the last bin"""
    k = np.minimum(np.floor(np.asarray(t, np.float32).astype(np.float64) * n).astype(np.int64), n - 1)
    out = np.zeros((n, 2))
    np.add.at(out[:, 0], k, np.asarray(l, np.float64))
    np.add.at(out[:, 1], k, 1.0)
    return out


VL_BLOCK, VLOSS_TILE = 256, 1024          # csrc/vloss_kernels.hip: accumulators of a batch-wide sum, rows of a tile


def _tree(acc):
    """block_sum: acc [..., 256] folded by sm[i] += sm[i + s] for i < s, s = 128, 64, .., 1 -> [...]"""
    acc = np.array(acc, np.float64)
    s = VL_BLOCK // 2
    while s:
        acc[..., :s] += acc[..., s:2 * s]
        s >>= 1
    return acc[..., 0]


def fixed_order_sum(v):
    """The sum launch_vloss_colsum takes of one column (include/ti_hip.h, Reduce): per tile of 1024 rows accumulator j adds rows
    4j .. 4j + 3 in order from +0.0, then the tree; across the tiles accumulator j adds tiles j, j + 256, .. in order, then the tree.
    Rows and tiles past the end are padded with +0.0, which an accumulator that started at +0.0 does not see."""
    v = np.asarray(v, np.float64).reshape(-1)
    tiles = max(1, -(-v.size // VLOSS_TILE))
    per = VLOSS_TILE // VL_BLOCK
    vv = np.zeros(tiles * VLOSS_TILE)
    vv[:v.size] = v
    vv = vv.reshape(tiles, VL_BLOCK, per)
    acc = np.zeros((tiles, VL_BLOCK))
    for k in range(per):
        acc += vv[:, :, k]
    partial = _tree(acc)
    rounds = -(-tiles // VL_BLOCK)
    pp = np.zeros(rounds * VL_BLOCK)
    pp[:tiles] = partial
    acc = np.zeros(VL_BLOCK)
    for row in pp.reshape(rounds, VL_BLOCK):
        acc += row
    return float(_tree(acc))


def time_bins_fixed_order(l, t, n):
    """time_bins in the order of vloss_tbins_kernel: per bin accumulator j adds the matching rows among j, j + 256, .. in order, then the tree"""
    l = np.asarray(l, np.float64)
    B = l.size
    k = np.minimum(np.floor(np.asarray(t, np.float32).astype(np.float64) * n).astype(np.int64), n - 1)
    acc, cnt = np.zeros((n, VL_BLOCK)), np.zeros((n, VL_BLOCK))
    for r0 in range(0, B, VL_BLOCK):
        j = np.arange(min(VL_BLOCK, B - r0))                # one row per accumulator and round: the pairs (bin, j) are distinct
        acc[k[r0:r0 + j.size], j] += l[r0:r0 + j.size]
        cnt[k[r0:r0 + j.size], j] += 1.0
    return np.stack([_tree(acc), _tree(cnt)], axis=1)


def dyadic_case(B, A, seed=0):
    """(x0, x1 [B, A, 3], t [B]) float32 on which one-sided interpolation and its column sums are exact in fp64: coordinates are
    integers in [-64, 64] over 16, t cycles through 1/4, 1/2, 3/4, so every product is a multiple of 2^-6 below 2^3 and a sum of 2^20
    of them still has fewer than 53 bits (tests/test_vloss_host.py checks this in rational arithmetic)."""
    rs = np.random.RandomState(seed)
    x0, x1 = (rs.randint(-64, 65, (B, A, 3)).astype(np.float32) / np.float32(16) for _ in range(2))
    return x0, x1, np.asarray([0.25, 0.5, 0.75], np.float32)[np.arange(B) % 3]


def philox4x32_10(counter, key):
    """counter [..., 4], key [2] uint32 -> [..., 4] uint32"""
    c = [np.asarray(counter[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m32, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=-1).astype(np.uint32)


def draw_u(seed, traj_offset, draw, B):
    """u [B] float32 = ((o[0] >> 9) + 0.5) 2^-23 of the Philox word of molecule traj_offset + b: exact, never 0 or 1"""
    ids = np.arange(B, dtype=np.uint64) + np.uint64(traj_offset)
    ctr = np.stack([ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32), np.full(B, draw, np.uint64), np.full(B, VLOSS_DOMAIN, np.uint64)], axis=-1)
    o = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return ((o[:, 0] >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def draw_t(t_dist, seed, traj_offset, draw, B):
    u = draw_u(seed, traj_offset, draw, B)
    if t_dist == "uniform":
        t = u
    elif t_dist == "beta_half":
        t = (np.sin(0.5 * np.pi * u.astype(np.float64)) ** 2).astype(np.float32)
    elif t_dist == "beta_2_1":
        t = np.sqrt(u.astype(np.float64)).astype(np.float32)
    else:
        raise ValueError(t_dist)
    return np.minimum(t, T_MAX)
