"""fp64 numpy restatement of the Z-matrix calls (include/ti_hip.h ti_obs_zmat, ti_obs_zmat_xyz) and of ZMatrix.from_bonds: the
oracle of the Z-matrix tests.  Inputs are taken as they are given to the device (fp32 values converted to fp64); nothing here runs
on a GPU.  order [A]: sorted atom s is the caller's atom order[s]; ref [A, 3] in sorted numbering."""
import numpy as np

PI32 = np.float32(np.pi)


def distance(x1, x2):
    return np.linalg.norm(np.asarray(x2, np.float64) - np.asarray(x1, np.float64), axis=-1)


def angle(x1, x2, x3):
    """the angle at x2 as atan2(|u x v|, u.v), [0, pi]"""
    u, v = np.asarray(x1, np.float64) - np.asarray(x2, np.float64), np.asarray(x3, np.float64) - np.asarray(x2, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(u, v), axis=-1), (u * v).sum(-1))


def torsion(x1, x2, x3, x4):
    x1, x2, x3, x4 = (np.asarray(v, np.float64) for v in (x1, x2, x3, x4))
    b1, b2, b3 = x2 - x1, x3 - x2, x4 - x3
    c23 = np.cross(b2, b3)
    return np.arctan2(np.linalg.norm(b2, axis=-1) * (b1 * c23).sum(-1), (np.cross(b1, b2) * c23).sum(-1))


def construct(x, order, ref):
    """z [B, A-1, 3] float64 of x [B, A, 3]: row s - 1 = (d, a, t) of sorted atom s; a = 0 in row 0, t = 0 in rows 0 and 1"""
    x = np.asarray(x, np.float64)[:, np.asarray(order)]
    A = x.shape[1]
    z = np.zeros((x.shape[0], A - 1, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(1, A):
            r1, r2, r3 = (int(v) for v in ref[s])
            z[:, s - 1, 0] = distance(x[:, s], x[:, r1])
            if s >= 2:
                z[:, s - 1, 1] = angle(x[:, s], x[:, r1], x[:, r2])
            if s >= 3:
                z[:, s - 1, 2] = torsion(x[:, r3], x[:, r2], x[:, r1], x[:, s])
    return z


def deconstruct(z, order, ref):
    """(x [B, A, 3] float64 in the caller's numbering, logdet [B], sum of |logdet terms| [B], conditioning [B, A] = |n| / |p2 - p1|
    before normalisation (1 for s < 3)) of z [B, A-1, 3]: NeRF placement in the canonical frame, no clamping"""
    z = np.asarray(z, np.float64)
    B, A = z.shape[0], z.shape[1] + 1
    X = np.zeros((B, A, 3))
    logdet, absum, cond = np.zeros(B), np.zeros(B), np.ones((B, A))
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(1, A):
            d, a, t = z[:, s - 1, 0], z[:, s - 1, 1], z[:, s - 1, 2]
            if s == 1:
                X[:, 1, 0] = d
            elif s == 2:
                r1 = int(ref[2][0])
                X[:, 2, 0] = X[:, r1, 0] - d * np.cos(a) if r1 != 0 else d * np.cos(a)
                X[:, 2, 1] = d * np.sin(a)
                term = np.log(np.abs(d))
                logdet, absum = logdet + term, absum + np.abs(term)
            else:
                p3, p2, p1 = (X[:, int(r)] for r in ref[s])
                e1 = p3 - p2
                e1 = e1 / np.linalg.norm(e1, axis=-1, keepdims=True)
                n = np.cross(p2 - p1, e1)
                ln = np.linalg.norm(n, axis=-1, keepdims=True)
                cond[:, s] = ln[:, 0] / np.linalg.norm(p2 - p1, axis=-1)
                n = n / ln
                e2 = np.cross(n, e1)
                sa = np.sin(a)
                X[:, s] = p3 - (d * np.cos(a))[:, None] * e1 + (d * sa * np.cos(t))[:, None] * e2 + (d * sa * np.sin(t))[:, None] * n
                t1, t2 = 2.0 * np.log(np.abs(d)), np.log(np.abs(sa))
                logdet, absum = logdet + (t1 + t2), absum + np.abs(t1) + np.abs(t2)
    out = np.zeros_like(X)
    out[:, np.asarray(order)] = X
    return out, logdet, absum, cond


def valid_mask(z):
    """correct_conf_indexes as a mask, compared in fp32: every row d > 0, 0 <= a <= pi32, -pi32 < t <= pi32 (NaN: 0)"""
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (z[..., 0] > 0) & (z[..., 1] >= 0) & (z[..., 1] <= PI32) & (z[..., 2] > -PI32) & (z[..., 2] <= PI32)
    return ok.all(axis=-1).astype(np.uint8)


def from_bonds(bonds, A, root=0):
    """(order [A], ref [A, 3]) by the rule of ZMatrix.from_bonds, written independently: a queue-based breadth-first search over an
    adjacency matrix; the references of sorted atom s are the first min(s, 3) distinct entries of its ancestors (nearest first)
    followed by the sorted atoms 0..s-1 in ascending order.  Unread slots are 0."""
    adj = np.zeros((A, A), bool)
    for i, j in np.asarray(bonds).reshape(-1, 2):
        adj[i, j] = adj[j, i] = True
    order, parent = [root], {root: -1}
    for a in order:                                   # the list grows while it is walked: a queue
        for c in np.flatnonzero(adj[a]):
            if int(c) not in parent:
                parent[int(c)] = a
                order.append(int(c))
    assert len(order) == A, "disconnected"
    rank = {a: s for s, a in enumerate(order)}
    ref = np.zeros((A, 3), np.int32)
    for s in range(1, A):
        chain, a = [], parent[order[s]]
        while a != -1:
            chain.append(rank[a])
            a = parent[a]
        rest = [r for r in range(s) if r not in chain]
        ref[s, :min(s, 3)] = (chain + rest)[:min(s, 3)]
    return np.asarray(order, np.int32), ref


def iqr_keep(logw, k):
    """filter_iqr of the reference on exp(logw - max) in fp64"""
    v = np.asarray(logw, np.float64)
    w = np.exp(v - v.max())
    q75, q25 = np.percentile(w, [75, 25])
    return ((w > q25 - k * (q75 - q25)) & (w < q75 + k * (q75 - q25))).astype(np.uint8)
