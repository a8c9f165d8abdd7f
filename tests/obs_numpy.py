"""fp64 numpy restatement of every observable the library computes (include/ti_hip.h ti_obs_*): the oracle of the observables tests.
Inputs are taken as they are given to the device (fp32 values converted to fp64), nothing here runs on a GPU."""
import numpy as np

RMSD, DIST, ANGLE, TORSION, COORD = 0, 1, 2, 3, 4


def kabsch_rmsd(x, ref, select=None):
    """x [B,A,3], ref [A,3]: minimal RMSD over proper rotations after centring, over the atoms with select != 0 (Kabsch by SVD,
    d = sign(det) keeps reflections out)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    if select is not None:
        keep = np.asarray(select) != 0
        x, ref = x[:, keep], ref[keep]
    n = x.shape[1]
    if n == 0:
        return np.full(x.shape[0], np.nan)
    x = x - x.mean(axis=1, keepdims=True)
    ref = ref - ref.mean(axis=0, keepdims=True)
    h = np.einsum("bai,aj->bij", x, ref)
    u, s, vt = np.linalg.svd(h)
    d = np.sign(np.linalg.det(u @ vt))
    s[:, -1] *= d
    e0 = (x ** 2).sum(axis=(1, 2)) + (ref ** 2).sum()
    return np.sqrt(np.maximum(e0 - 2.0 * s.sum(axis=1), 0.0) / n)


def rmsd_scale(x, ref, select=None):
    """sqrt(e0 / count): the coordinate scale the RMSD bound is stated in (e0 = |x|^2 + |ref|^2 after centring)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    if select is not None:
        keep = np.asarray(select) != 0
        x, ref = x[:, keep], ref[keep]
    x = x - x.mean(axis=1, keepdims=True)
    ref = ref - ref.mean(axis=0, keepdims=True)
    return np.sqrt(((x ** 2).sum(axis=(1, 2)) + (ref ** 2).sum()) / max(x.shape[1], 1))


def distance(x1, x2):
    return np.linalg.norm(np.asarray(x2, np.float64) - np.asarray(x1, np.float64), axis=-1)


def angle(x1, x2, x3):
    """the angle at x2, [0, pi]; the cosine is clipped to [-1, 1] (collinear triples round past it)"""
    a, b = np.asarray(x1, np.float64) - np.asarray(x2, np.float64), np.asarray(x3, np.float64) - np.asarray(x2, np.float64)
    c = (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
    return np.arccos(np.clip(c, -1.0, 1.0))


def torsion(x1, x2, x3, x4):
    x1, x2, x3, x4 = (np.asarray(v, np.float64) for v in (x1, x2, x3, x4))
    b1, b2, b3 = x2 - x1, x3 - x2, x4 - x3
    c23 = np.cross(b2, b3)
    y = np.linalg.norm(b2, axis=-1) * (b1 * c23).sum(-1)
    xx = (np.cross(b1, b2) * c23).sum(-1)
    return np.arctan2(y, xx)


def collective_variables(x, desc, ref=None, select=None, n_atoms=None):
    """cv [B,K] float64 of x [B,A,3] (or [B,d] for COORD) for desc [K][5]; n_atoms [B]: real atoms per molecule (pads -> NaN, RMSD
    over the real selected atoms)."""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    out = np.zeros((B, len(desc)))
    for k, (kind, i, j, kk, l) in enumerate(np.asarray(desc).tolist()):
        if kind == COORD:
            out[:, k] = x.reshape(B, -1)[:, i]
        elif kind == RMSD:
            if n_atoms is None:
                out[:, k] = kabsch_rmsd(x, ref, select)
            else:
                for b in range(B):
                    n = int(n_atoms[b])
                    out[b, k] = kabsch_rmsd(x[b:b + 1, :n], np.asarray(ref)[:n], None if select is None else np.asarray(select)[:n])[0]
        else:
            idx = [i, j, kk, l][:{DIST: 2, ANGLE: 3, TORSION: 4}[kind]]
            fn = {DIST: distance, ANGLE: angle, TORSION: torsion}[kind]
            with np.errstate(invalid="ignore", divide="ignore"):
                out[:, k] = fn(*(x[:, a] for a in idx))
            if n_atoms is not None:
                out[np.asarray(n_atoms) <= max(idx), k] = np.nan
    return out


def importance_weights(logw):
    """(w normalised, ess) with the max shift; ess = (sum w)^2 / sum w^2 (the reference's calc_ESS)."""
    logw = np.asarray(logw, np.float64)
    w = np.exp(logw - logw.max())
    return w / w.sum(), float(np.square(w.sum()) / np.square(w).sum())


def bin_edges(bins, lo, hi):
    return lo + ((hi - lo) * np.arange(bins + 1, dtype=np.float64)) / bins


def bin_index(values, bins, lo, hi):
    """bin of every value: 0..bins-1 for e_k <= v < e_k+1 (a value on an interior edge goes up), bins: below lo, bins + 1: hi or above,
    bins + 2: not finite"""
    v = np.asarray(values, np.float64)
    e = bin_edges(bins, lo, hi)
    idx = np.searchsorted(e[1:-1], v, side="right")              # number of interior edges <= v
    idx = np.where(v < lo, bins, np.where(v >= hi, bins + 1, idx))
    return np.where(np.isfinite(v), idx, bins + 2)


def weighted_histogram(values, logw, bins, lo, hi):
    """(hist [bins], tails [3] = below, above, nonfinite); logw None: weights 1 / B"""
    v = np.asarray(values, np.float64)
    w = np.full(v.size, 1.0 / v.size) if logw is None else importance_weights(logw)[0]
    full = np.bincount(bin_index(v, bins, lo, hi), weights=w, minlength=bins + 3)
    return full[:bins], full[bins:]


def edge_clearance(values, bins, lo, hi):
    """smallest distance of every finite value to a bin edge (lo and hi included)"""
    v = np.asarray(values, np.float64)
    return np.abs(v[:, None] - bin_edges(bins, lo, hi)[None, :]).min(axis=1)


def free_energy_profile(x, logw, bins=80, lo=-2.5, hi=2.5):
    hist, _ = weighted_histogram(np.asarray(x).reshape(-1), logw, bins, lo, hi)
    with np.errstate(divide="ignore"):
        p = hist / (hist.sum() * (hi - lo) / bins)
        return np.where(p > 0, -np.log(p), np.inf)
