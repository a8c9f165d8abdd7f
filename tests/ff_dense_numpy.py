"""Dense synthetic force fields: bonded tables of any length over random distinct atoms, for the table edges that no tree of 25 atoms
reaches (chunks of 64 terms, empty tables in front of full ones, the caps 64 / 128 / 512, one atom in every term of a chunk).  The
particles, the pair table and the geometries are those of the tree species of tests/ff_numpy.py; only the bonded tables are replaced.
CASES names the ones tests/test_ff_forces_host.py conditions and tests/test_gpu_ff_edges.py and tests/test_gpu_md_edges.py run.  Nothing
here runs on a GPU or needs the package."""
import functools

import numpy as np

import ff_numpy as fn

ANGLE_MIN, ANGLE_MAX = np.deg2rad(25.0), np.deg2rad(155.0)     # acos and the torsion's 1 / |m|^2 lose digits outside


def _distinct(rs, n, slots, A):
    """[n, slots] rows of distinct atoms, uniformly"""
    return np.argsort(rs.random_sample((n, A)), axis=1)[:, :slots]


def _inside(p, i, j, k):
    """[n] bool: the angle (i, j, k) lies in [25, 155] degrees in every molecule of p [B, A, 3]"""
    th = fn._angle(p, i, j, k, np.float64)
    return ((th >= ANGLE_MIN) & (th <= ANGLE_MAX)).all(axis=0)


def _draw(rs, n, slots, A, keep):
    """n rows of `slots` distinct atoms that keep() accepts, in the order drawn (a row may repeat: two terms on the same atoms)"""
    out = np.zeros((0, slots), np.int64)
    if n == 0:
        return out.astype(np.int32)
    if slots > A:
        raise ValueError(f"a term of {slots} atoms needs A >= {slots}")
    for _ in range(200):
        cand = _distinct(rs, 4 * n + 64, slots, A)
        out = np.concatenate([out, cand[keep(cand)]])
        if len(out) >= n:
            return out[:n].astype(np.int32)
    raise RuntimeError(f"no {n} acceptable terms of {slots} atoms among {A}")


def dense_forcefield(A, nb, na, nt, B, seed=0, hub=False):
    """(ff dict, x [B, A, 3] fp32, to_nm): the particles, the exceptions (so the pair table) and B geometries of
    fn.synthetic_forcefield(A, seed) / fn.synthetic_geometry, with the bonded tables replaced by nb bonds, na angles and nt torsions over
    random distinct atoms.  An angle (i, j, k) is taken only if it lies in [25, 155] degrees in every one of the B molecules, a torsion
    only if both of its bond angles (i, j, k) and (j, k, l) do.  Parameters from synthetic_forcefield's ranges, periodicity 1 .. 6, phase
    0 or pi.  hub=True: slot 0 of every bond is atom 0 and slot 1 comes from the atoms 1 .. A // 2, so that atom 0 sits in every term of
    a bond chunk and the upper half of the atoms in none.  A count may be 0.  Deterministic in its arguments."""
    tree = fn.synthetic_forcefield(A, seed)
    x, to_nm = fn.synthetic_geometry(tree, B, seed=seed + 1)
    p = x.astype(np.float64) * to_nm
    rs = np.random.RandomState(7919 * A + 104729 * seed + 31 * nb + 17 * na + nt + (1 << 20) * bool(hub))
    if hub:
        if nb and A < 3:
            raise ValueError("a hub needs A >= 3")
        bonds = np.stack([np.zeros(nb, np.int64), rs.randint(1, A // 2 + 1, nb)], axis=1).astype(np.int32)
    else:
        bonds = _draw(rs, nb, 2, A, lambda c: np.ones(len(c), bool))
    angles = _draw(rs, na, 3, A, lambda c: _inside(p, c[:, 0], c[:, 1], c[:, 2]))
    tors = _draw(rs, nt, 4, A, lambda c: _inside(p, c[:, 0], c[:, 1], c[:, 2]) & _inside(p, c[:, 1], c[:, 2], c[:, 3]))
    ff = dict(bond_idx=bonds.reshape(-1, 2), bond_par=np.stack([rs.uniform(0.10, 0.16, nb), rs.uniform(1.5e5, 4e5, nb)], axis=1),
              angle_idx=angles.reshape(-1, 3), angle_par=np.stack([rs.uniform(1.7, 2.1, na), rs.uniform(300.0, 700.0, na)], axis=1),
              torsion_idx=tors.reshape(-1, 4),
              torsion_par=np.stack([rs.randint(1, 7, nt).astype(np.float64), rs.randint(0, 2, nt) * np.pi, rs.uniform(0.5, 10.0, nt)], axis=1),
              particles=tree["particles"], exceptions=tree["exceptions"], coulomb=fn.COULOMB)
    return ff, x, to_nm


def incidence(ff, A):
    """[n_chunks, A] int: how many (term, slot) entries atom a has in chunk q -- bond chunks, then angle chunks, then torsion chunks,
    64 terms each, an empty table no chunk: the lengths of the lists the forces are gathered through"""
    rows = []
    for key in ("bond_idx", "angle_idx", "torsion_idx"):
        idx = np.asarray(ff[key], np.int64)
        for base in range(0, len(idx), 64):
            rows.append(np.bincount(idx[base:base + 64].reshape(-1), minlength=A))
    return np.array(rows, np.int64).reshape(-1, A)


B_DENSE = 9                       # batches of 1, 5 and 9: one molecule; a workgroup's four and one; two workgroups and one
# name -> (A, bonds, angles, torsions, hub)
CASES = {
    "all_caps": (25, 64, 128, 512, False),          # every LDS array and the offset list at their largest; 1 + 2 + 8 chunks
    "angles_2nd": (25, 24, 65, 64, False),          # the chunk number after a two-chunk angle table; torsions exactly one full chunk
    "no_bonds": (25, 0, 65, 65, False),             # the angles start at chunk 0 after an empty table
    "tors_only": (25, 0, 0, 129, False),            # two empty tables in front
    "pairs_only": (24, 0, 0, 0, False),             # no chunk at all; even A
    "hub": (22, 64, 64, 65, True),                  # 64 entries of one atom in one chunk, atoms with none; 3A = 66
    "below_half": (21, 63, 128, 129, False),        # 3A = 63: no second component; odd h; a bond chunk one short of full
    "three_atoms": (3, 2, 3, 0, False),             # h = 2, lanes 6 .. 63 idle in the pair stage
}


@functools.lru_cache(maxsize=None)
def dense_case(name):
    """(ff dict, x [B_DENSE, A, 3] fp32, to_nm) of CASES[name], generated once"""
    A, nb, na, nt, hub = CASES[name]
    return dense_forcefield(A, nb, na, nt, B_DENSE, seed=0, hub=hub)
