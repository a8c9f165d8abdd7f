"""Z-matrix (internal) coordinates on the GPU (include/ti_hip.h ti_obs_zmat, ti_obs_zmat_xyz, ti_obs_hist_cols): what the reference's
mdqm9/analysis/utils/z_matrix.py does around mdqm9/analysis/results_00031.py.

    zm = ZMatrix(order, ref_atoms)              # the reference's atom_order and ref_atoms, or ZMatrix.from_bonds(bonds, A)
    z = zmatrix(engine, x, zm)                  # construct_z_matrix_batch(x[:, order], ref_atoms): [B, A-1, 3] rows (d, a, t)
    x, logdet, valid = zmatrix_xyz(engine, z, zm, logdet=True, valid=True)      # deconstruct_z_matrix_batch(jacobian=True),
                                                                                # correct_conf_indexes as a mask
    torsions(z), bond_angles(z), bond_lengths(z)                                # gen_torsions / gen_bond_angles / gen_bond_lengths
    keep = iqr_keep(logw, k)                                                    # sensititvity.filter_iqr on exp(logw - max)
    hist, tails, ranges = zmatrix_marginals(z, logw, keep)                      # the weighted marginals of all 3A - 6 coordinates

``order`` [A] is a permutation: sorted atom s is the caller's atom order[s].  ``ref_atoms`` [A, 3] is in sorted numbering:
ref_atoms[s] = (r1, r2, r3) gives sorted atom s the distance to r1, the angle (s, r1, r2) at r1 and the torsion (r3, r2, r1, s).  Only
ref_atoms[s][0] is read for s >= 1, [s][1] for s >= 2 and [s][2] for s >= 3; the slots read must be < s and distinct.

Deviations from the reference, on purpose: the angle is atan2(|u x v|, u.v) in fp64 (ti_obs_cv's ANGLE) instead of an fp32 acos; the
log-determinant is the closed form log|d_2| + sum_{s>=3} (2 log|d_s| + log|sin a_s|) of the reference's 2x2 and 3x3 determinants;
all arithmetic is fp64 on the fp32 inputs.  ``ZMatrix.from_bonds`` is a rule of this build (see there): parity with the reference's
rdkit-based sort_atoms.compute_atom_order_and_references_groups is NOT pinned -- pass its atom_order / ref_atoms to ZMatrix to
reproduce a reference run.
"""
from __future__ import annotations

import collections

import numpy as np

from . import _lib


def check_topology(order, ref_atoms, A=None):
    """(order [A] int32, ref [A, 3] int32) validated exactly as ti_obs_zmat validates them; order None: the identity.  Slots that are
    never read are returned as 0."""
    ref = np.asarray(ref_atoms)
    if ref.ndim != 2 or ref.shape[1] != 3 or ref.dtype.kind not in "iu":
        raise ValueError(f"ref_atoms must be an integer array [A, 3], got {ref.dtype} {ref.shape}")
    n = int(ref.shape[0])
    if A is not None and n != int(A):
        raise ValueError(f"ref_atoms must have A = {int(A)} rows, got {n}")
    if not _lib.ZMAT_MIN_ATOMS <= n <= _lib.ZMAT_MAX_ATOMS:
        raise ValueError(f"a Z-matrix needs {_lib.ZMAT_MIN_ATOMS} <= A <= {_lib.ZMAT_MAX_ATOMS}, got A = {n}")
    if order is None:
        order = np.arange(n)
    order = np.asarray(order)
    if order.shape != (n,) or order.dtype.kind not in "iu" or sorted(order.tolist()) != list(range(n)):
        raise ValueError(f"order must be a permutation of 0..{n - 1}")
    out = np.zeros((n, 3), np.int32)
    for s in range(1, n):
        for j in range(min(s, 3)):
            r = int(ref[s, j])
            if not 0 <= r < s:
                raise ValueError(f"ref_atoms[{s}][{j}] = {r} is not an earlier sorted atom")
            if r in ref[s, :j].tolist():
                raise ValueError(f"ref_atoms[{s}] repeats atom {r}")
            out[s, j] = r
    return np.ascontiguousarray(order, np.int32), out


class ZMatrix:
    """A Z-matrix topology: ``order`` [A] and ``ref`` [A, 3] int32 (module docstring), validated as the library validates them."""

    def __init__(self, order, ref_atoms):
        self.order, self.ref = check_topology(order, ref_atoms)
        self.A = int(self.ref.shape[0])

    @property
    def n_internal(self):
        """3A - 6 for A >= 3 (1 for A = 2): the coordinates that are not structural zeros"""
        return (self.A - 1) + max(self.A - 2, 0) + max(self.A - 3, 0)

    @classmethod
    def from_bonds(cls, bonds, A, root=0):
        """A topology from a bond list [[i, j], ...] over atoms 0..A-1 (one connected molecule): breadth-first from ``root``, the
        neighbours of an atom in ascending index; ``order`` is the visit order; the references of sorted atom s are the first three
        distinct entries of [its BFS parent, the parent's parent, ... up to the root, then the atoms placed before s in ascending
        sorted index].  This is a rule of this build: it is not the reference's rdkit-based atom sorter, and it does not look at the
        geometry -- references that are collinear in the samples (a linear group) are the caller's to avoid by passing order and
        ref_atoms explicitly."""
        A = int(A)
        if not _lib.ZMAT_MIN_ATOMS <= A <= _lib.ZMAT_MAX_ATOMS:
            raise ValueError(f"a Z-matrix needs {_lib.ZMAT_MIN_ATOMS} <= A <= {_lib.ZMAT_MAX_ATOMS}, got A = {A}")
        b = np.asarray(bonds)
        if b.ndim != 2 or b.shape[1] != 2 or b.dtype.kind not in "iu":
            raise ValueError(f"bonds must be an integer array [n, 2], got {b.dtype} {b.shape}")
        if b.size and (b.min() < 0 or b.max() >= A or (b[:, 0] == b[:, 1]).any()):
            raise ValueError(f"bonds must join two different atoms of 0..{A - 1}")
        if isinstance(root, bool) or int(root) != root or not 0 <= int(root) < A:
            raise ValueError(f"root must be an atom of 0..{A - 1}, got {root!r}")
        nbrs = [set() for _ in range(A)]
        for i, j in b.tolist():
            nbrs[i].add(j); nbrs[j].add(i)
        order, parent, rank = [int(root)], {int(root): None}, {int(root): 0}
        head = 0
        while head < len(order):
            a = order[head]; head += 1
            for c in sorted(nbrs[a]):
                if c not in parent:
                    parent[c] = a; rank[c] = len(order); order.append(c)
        if len(order) != A:
            raise ValueError(f"the bonds do not connect all {A} atoms to root {int(root)} ({len(order)} reached)")
        ref = np.zeros((A, 3), np.int64)
        for s in range(1, A):
            cand, a = [], parent[order[s]]
            while a is not None:
                cand.append(rank[a]); a = parent[a]
            cand += [r for r in range(s) if r not in cand]
            ref[s, :min(s, 3)] = cand[:min(s, 3)]
        return cls(order, ref)

    def descriptors(self):
        """The ti_obs_cv descriptors of all 3 (A - 1) entries of z, row-major, on the caller's atoms; the structural zeros are None."""
        o, r, out = self.order, self.ref, []
        for s in range(1, self.A):
            out.append(("dist", int(o[s]), int(o[r[s, 0]])))
            out.append(("angle", int(o[s]), int(o[r[s, 0]]), int(o[r[s, 1]])) if s >= 2 else None)
            out.append(("torsion", int(o[r[s, 2]]), int(o[r[s, 1]]), int(o[r[s, 0]]), int(o[s])) if s >= 3 else None)
        return out


def torsions(z):
    """z[:, 2:, 2] (results_00031.py gen_torsions)"""
    return z[:, 2:, 2]


def bond_angles(z):
    """z[:, 1:, 1] (gen_bond_angles)"""
    return z[:, 1:, 1]


def bond_lengths(z):
    """z[:, :, 0] (gen_bond_lengths)"""
    return z[:, :, 0]


def iqr_keep(logw, k):
    """keep [B] uint8: the reference's sensititvity.filter_iqr(weights, k) restated on the host for weights = exp(logw - max logw) in
    fp64 -- q25, q75 by numpy's default percentile, keep where q25 - k iqr < w < q75 + k iqr (both strict).  k None: everything.
    The filter is invariant under the positive scale exp(-max), so this is the reference's mask of exp(logw) wherever that does
    not overflow."""
    v = np.asarray(logw.detach().cpu().numpy() if hasattr(logw, "data_ptr") else logw, np.float64).reshape(-1)
    if v.size < 1:
        raise ValueError("logw must be non-empty")
    if k is None:
        return np.ones(v.shape, np.uint8)
    if isinstance(k, bool) or not (np.isfinite(k) and k > 0):
        raise ValueError(f"k must be finite and > 0 (or None), got {k!r}")
    if not np.isfinite(v).all():
        raise ValueError(f"non-finite logw at index {int(np.flatnonzero(~np.isfinite(v))[0])}")
    w = np.exp(v - v.max())
    q75, q25 = np.percentile(w, [75, 25])
    iqr = q75 - q25
    return ((w > q25 - k * iqr) & (w < q75 + k * iqr)).astype(np.uint8)


def _as_zmatrix(zm):
    if isinstance(zm, ZMatrix):
        return zm
    if isinstance(zm, (tuple, list)) and len(zm) == 2:
        return ZMatrix(*zm)
    raise TypeError("expected a ZMatrix (or an (order, ref_atoms) pair)")


def zmatrix(engine, x, zm, out=None):
    """z [B, A-1, 3] float32 of x [B, A, 3] on a PainnEngine of the species (ti_obs_zmat); lives where x lives."""
    return engine.zmatrix(x, _as_zmatrix(zm), out=out)


def zmatrix_xyz(engine, z, zm, logdet=False, valid=False):
    """x [B, A, 3] float32 of z [B, A-1, 3] in the caller's atom numbering and the reference's canonical frame (ti_obs_zmat_xyz); with
    logdet and / or valid also log|det J| [B] float64 and the validity mask [B] uint8, as a tuple in that order.  Lives where z lives."""
    return engine.zmatrix_xyz(z, _as_zmatrix(zm), logdet=logdet, valid=valid)


ZMarginals = collections.namedtuple("ZMarginals", "hist tails ranges")
ZMarginals.__doc__ = """hist [3A-6, bins] and tails [3A-6, 3] float64 (the weight per bin; below, at or above the range, non-finite), ranges
[3A-6, 2]: rows in the order bond lengths (A - 1), bond angles (A - 2), torsions (A - 3)."""


def marginal_columns(A):
    """The columns of z.reshape(B, 3 (A - 1)) that are internal coordinates, in the order lengths, angles, torsions."""
    rows = np.arange(A - 1)
    return np.concatenate([3 * rows, 3 * rows[1:] + 1, 3 * rows[2:] + 2]).astype(np.int64)


def zmatrix_marginals(z, logw=None, keep=None, bins=64, length_range=(0.0, 4.0), engine=None):
    """The weighted marginal histograms of all 3A - 6 internal coordinates of z [B, A-1, 3] in ONE ti_obs_hist_cols call (the two
    weight reductions are done once, not once per column): bond lengths on ``length_range`` (in the units of z), angles on [0, pi],
    torsions on [-pi, pi], `bins` equal bins each, pi the fp64 value.  A value equal to the upper end of its range lands in the upper
    tail, not in the last bin: an fp32 torsion of exactly (float)pi -- which is above the fp64 pi -- is counted in tails[:, 1].
    logw [B] float32 (None: uniform) as in observables.weighted_histogram; keep [B] uint8 (e.g. ``iqr_keep``): entries with keep == 0
    get weight 0 and the weights are normalised over the kept entries only."""
    from . import observables as _obs
    if len(z.shape) != 3 or int(z.shape[2]) != 3 or int(z.shape[1]) < 1:
        raise ValueError(f"z must be [B, A-1, 3], got {tuple(z.shape)}")
    B, A = int(z.shape[0]), int(z.shape[1]) + 1
    bins, llo, lhi = _obs.check_bins(bins, length_range)
    K = 3 * (A - 1)
    lo, hi = np.empty(K), np.empty(K)
    lo[0::3], hi[0::3] = llo, lhi
    lo[1::3], hi[1::3] = 0.0, np.pi
    lo[2::3], hi[2::3] = -np.pi, np.pi
    eng = engine or _obs._service_engine(_obs._device_of(z, logw))
    hist, tails = eng.hist_cols(z.reshape(B, K), logw, keep, bins, lo, hi)
    cols = marginal_columns(A)
    return ZMarginals(hist[cols], tails[cols], np.stack([lo[cols], hi[cols]], axis=1))
