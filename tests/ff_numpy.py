"""numpy restatement of the force-field energies the library computes (include/ti_hip.h ti_obs_ff_energy), written from the header's
formulas: the oracle of tests/test_forcefield.py and tests/test_gpu_forcefield.py and the CPU side of tools/ff_bench.py.  It runs in
any float type (fp64, np.longdouble for the conditioning check).  Also a deterministic synthetic force field for A atoms and a
matching geometry generator.  Nothing here runs on a GPU or needs the package."""
import numpy as np

R_GAS = 0.00831446261815324          # kJ / (mol K)
COULOMB = 138.935456                 # OpenMM's ONE_4PI_EPS0
TERMS = ("bond", "angle", "torsion", "pair")


def pair_row(i, j, A):
    return i * (2 * A - i - 1) // 2 + (j - i - 1)


def pair_table(ff, A):
    """[A (A - 1) / 2, 3] (qq, sigma, eps): Lorentz-Berthelot, then the exceptions, rows in (i, j) order with i < j"""
    q, sig, eps = (np.asarray(ff["particles"], np.float64)[:, c] for c in range(3))
    out = np.zeros((A * (A - 1) // 2, 3))
    for i in range(A):
        for j in range(i + 1, A):
            out[pair_row(i, j, A)] = q[i] * q[j], (sig[i] + sig[j]) / 2.0, np.sqrt(eps[i] * eps[j])
    for i, j, qq, s, e in np.asarray(ff["exceptions"], np.float64).reshape(-1, 5):
        i, j = int(min(i, j)), int(max(i, j))
        out[pair_row(i, j, A)] = qq, s, e
    return out


def _angle(p, i, j, k, ft):
    u, v = p[:, i] - p[:, j], p[:, k] - p[:, j]
    c = (u * v).sum(-1) / (np.sqrt((u * u).sum(-1)) * np.sqrt((v * v).sum(-1)))
    return np.arccos(np.clip(c, ft(-1), ft(1)))                 # np.clip keeps a NaN


def _torsion(p, i, j, k, l):
    b1, b2, b3 = p[:, j] - p[:, i], p[:, k] - p[:, j], p[:, l] - p[:, k]
    c23 = np.cross(b2, b3)
    return np.arctan2(np.sqrt((b2 * b2).sum(-1)) * (b1 * c23).sum(-1), (np.cross(b1, b2) * c23).sum(-1))


def bond_energy(r, r0, k):
    dr = r - r0
    return k * dr * dr / 2


def angle_energy(theta, theta0, k):
    return bond_energy(theta, theta0, k)                        # the same harmonic form


def torsion_energy(phi, n, phase, k):
    return k * (1 + np.cos(n * phi - phase))


def pair_energy(r, qq, sigma, eps, coulomb=COULOMB):
    """4 eps s (s - 1) + coulomb qq / r, s = (sigma / r)^6; the Lennard-Jones part only with eps > 0 and sigma > 0, the Coulomb part
    only with qq != 0; where the wall is +inf (r = 0) it wins over an attractive charge product"""
    ft = np.result_type(r, qq).type
    s6 = (sigma / r) ** 2
    s6 = s6 * s6 * s6
    lj = np.where((eps > 0) & (sigma > 0), ft(4) * eps * s6 * (s6 - ft(1)), ft(0))
    cl = np.where(qq != 0, ft(coulomb) * qq / r, ft(0))
    return np.where(lj == np.inf, lj, lj + cl)


def term_arrays(x, to_nm, ff, pairs, ft=np.float64):
    """The four per-term arrays [B, n_table] of x [B, A, 3] fp32 at positions x * to_nm, in kJ/mol, in the float type ft; the pair
    array holds the evaluated rows only (qq != 0 or eps != 0), in row order."""
    p = np.asarray(x, np.float32).astype(ft) * ft(np.float64(to_nm))
    B, A = p.shape[:2]
    bi, bp = np.asarray(ff["bond_idx"], np.int64).reshape(-1, 2), np.asarray(ff["bond_par"], np.float64).reshape(-1, 2).astype(ft)
    ai, ap = np.asarray(ff["angle_idx"], np.int64).reshape(-1, 3), np.asarray(ff["angle_par"], np.float64).reshape(-1, 2).astype(ft)
    ti, tp = np.asarray(ff["torsion_idx"], np.int64).reshape(-1, 4), np.asarray(ff["torsion_par"], np.float64).reshape(-1, 3).astype(ft)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = p[:, bi[:, 1]] - p[:, bi[:, 0]]
        e_bond = bond_energy(np.sqrt((d * d).sum(-1)), bp[:, 0], bp[:, 1])
        e_angle = angle_energy(_angle(p, ai[:, 0], ai[:, 1], ai[:, 2], ft), ap[:, 0], ap[:, 1])
        e_tors = torsion_energy(_torsion(p, ti[:, 0], ti[:, 1], ti[:, 2], ti[:, 3]), tp[:, 0], tp[:, 1], tp[:, 2])
        ii, jj = np.triu_indices(A, 1)
        pr = np.asarray(pairs, np.float64).reshape(-1, 3)
        live = (pr[:, 0] != 0) | (pr[:, 2] != 0)
        ii, jj, pr = ii[live], jj[live], pr[live].astype(ft)
        d = p[:, jj] - p[:, ii]
        e_pair = pair_energy(np.sqrt((d * d).sum(-1)), pr[:, 0], pr[:, 1], pr[:, 2], ft(np.float64(ff.get("coulomb", COULOMB))))
    return [np.asarray(e, ft).reshape(B, -1) for e in (e_bond, e_angle, e_tors, e_pair)]


def energies(x, to_nm, ff, pairs=None, T=None, ft=np.float64):
    """(E [B], sums [B, 4], S [B, 4], arrays): the four term sums and their total ((bond + angle) + torsion) + pair -- each divided by
    R T_b when T [B] is given -- and S = sum over a column's evaluated terms of (1 + |term|) in the same unit, the scale the
    tolerances are stated in (its row sum is the scale of E)."""
    A = np.asarray(x).shape[1]
    pairs = pair_table(ff, A) if pairs is None else pairs
    arrays = term_arrays(x, to_nm, ff, pairs, ft)
    rt = None if T is None else ft(R_GAS) * np.asarray(T, np.float32).astype(ft)
    sums = np.stack([a.sum(-1) for a in arrays], axis=1)
    S = np.stack([(1.0 + np.abs(np.nan_to_num(a.astype(np.float64), posinf=0.0, neginf=0.0))).sum(-1) for a in arrays], axis=1)
    if rt is not None:
        sums = sums / rt[:, None]
    E = ((sums[:, 0] + sums[:, 1]) + sums[:, 2]) + sums[:, 3]
    return E, sums, S, arrays


# ---- synthetic species ---------------------------------------------------------------------------------------------------------
def synthetic_forcefield(A, seed=0, max_degree=6, parents=None):
    """A deterministic GAFF-shaped force field for A atoms as a dict of arrays (the fields of forcefield.ForceField): a random tree
    as bonds (new atoms prefer parents that already have neighbours, up to max_degree; or parents [A - 1] as given), every angle and proper torsion the tree
    implies, a second term of another periodicity behind every torsion whose table index is odd, phases in {0, pi}, charges that sum
    to 0, the 1-2 and 1-3 pairs zeroed and the 1-4 pairs scaled by 1 / 1.2 (charge product) and 1 / 2 (eps) as exceptions."""
    rs = np.random.RandomState(1000 * A + seed)
    nbrs = [[] for _ in range(A)]
    bonds = []
    for a in range(1, A):
        cand = [c for c in range(a) if len(nbrs[c]) < max_degree]
        w = np.array([(1.0 + len(nbrs[c])) ** 2 for c in cand])
        par = cand[int(rs.choice(len(cand), p=w / w.sum()))]
        par = par if parents is None else int(parents[a - 1])
        bonds.append((par, a)); nbrs[par].append(a); nbrs[a].append(par)
    angles = [(i, j, k) for j in range(A) for x, i in enumerate(nbrs[j]) for k in nbrs[j][x + 1:]]
    base = [(i, j, k, l) for j, k in bonds for i in nbrs[j] if i != k for l in nbrs[k] if l != j]
    tors, tpar = [], []
    for q in base:
        n = int(rs.randint(1, 7))
        terms = [n]
        if len(tors) % 2 == 1:
            terms.append(n % 6 + 1)
        for m in terms:
            tors.append(q)
            tpar.append((float(m), float(rs.randint(0, 2)) * np.pi, rs.uniform(0.5, 10.0)))
    q = rs.standard_normal(A) * 0.3
    q -= q.mean()
    particles = np.stack([q, rs.uniform(0.1, 0.35, A), rs.uniform(0.05, 0.5, A)], axis=1)
    dist = np.full((A, A), 99, np.int64)                        # tree distances by breadth-first search
    for s in range(A):
        dist[s, s], frontier = 0, [s]
        while frontier:
            nxt = []
            for u in frontier:
                for v in nbrs[u]:
                    if dist[s, v] == 99:
                        dist[s, v] = dist[s, u] + 1; nxt.append(v)
            frontier = nxt
    exc = []
    for i in range(A):
        for j in range(i + 1, A):
            if dist[i, j] <= 2:
                exc.append((i, j, 0.0, 1.0, 0.0))
            elif dist[i, j] == 3:
                exc.append((i, j, q[i] * q[j] / 1.2, (particles[i, 1] + particles[j, 1]) / 2, np.sqrt(particles[i, 2] * particles[j, 2]) / 2))
    nb, na = len(bonds), len(angles)
    return dict(bond_idx=np.array(bonds, np.int32).reshape(-1, 2), bond_par=np.stack([rs.uniform(0.10, 0.16, nb), rs.uniform(1.5e5, 4e5, nb)], axis=1),
                angle_idx=np.array(angles, np.int32).reshape(-1, 3),
                angle_par=np.stack([rs.uniform(1.7, 2.1, na), rs.uniform(300.0, 700.0, na)], axis=1).reshape(-1, 2),
                torsion_idx=np.array(tors, np.int32).reshape(-1, 4), torsion_par=np.array(tpar, np.float64).reshape(-1, 3),
                particles=particles, exceptions=np.array(exc, np.float64).reshape(-1, 5), coulomb=COULOMB)


def chain_forcefield(A, seed=0):
    """synthetic_forcefield on the chain 0 - 1 - ... - A-1"""
    return synthetic_forcefield(A, seed, parents=list(range(A - 1)))


def synthetic_geometry(ff, B, seed=0, scale=7.3):
    """(x [B, A, 3] float32 model coordinates, to_nm = 1 / scale): every molecule grown along the tree edges with random bond lengths
    of 0.10 - 0.16 nm, a new atom rejected while it is closer than 0.09 nm to a placed one or makes an angle beyond 160 degrees at its
    parent (acos loses digits there)."""
    rs = np.random.RandomState(seed)
    bonds = np.asarray(ff["bond_idx"]).reshape(-1, 2)
    A = int(np.asarray(ff["particles"]).shape[0])
    nbrs = [[] for _ in range(A)]
    x = np.zeros((B, A, 3))
    for b in range(B):
        for lst in nbrs:
            lst.clear()
        for par, a in bonds:
            for _ in range(10000):
                v = rs.standard_normal(3)
                v /= np.linalg.norm(v)
                pos = x[b, par] + v * rs.uniform(0.10, 0.16)
                ok = a == 0 or np.linalg.norm(x[b, :a] - pos, axis=1).min() >= 0.09
                for o in nbrs[par]:
                    u = x[b, o] - x[b, par]
                    ok = ok and (u @ v) / np.linalg.norm(u) > np.cos(np.deg2rad(160.0))
                if ok:
                    break
            else:
                raise RuntimeError("no room for the next atom")
            x[b, a] = pos
            nbrs[par].append(a)
    x -= x.mean(axis=1, keepdims=True)
    return (x * scale).astype(np.float32), 1.0 / scale
