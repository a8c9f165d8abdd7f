"""numpy restatement of the force-field forces and of the Langevin integrator the library computes (include/ti_hip.h ti_obs_ff_forces,
ti_obs_ff_langevin), written from the header's formulas next to the energy restatement (tests/ff_numpy.py): the oracle of
tests/test_ff_forces_host.py, tests/test_gpu_ff_forces.py, tests/test_gpu_md.py and their edge files (tests/test_gpu_ff_edges.py,
tests/test_gpu_md_edges.py).  It runs in any float type (fp64, np.longdouble for
the conditioning checks).  Nothing here runs on a GPU or needs the package."""
import numpy as np

import ff_numpy as fn


def masses_for(ff):
    """[A] float64: 12.0 everywhere except 1.008 on the leaf atoms (one bond) of a species with more than two atoms"""
    A = int(np.asarray(ff["particles"]).shape[0])
    deg = np.bincount(np.asarray(ff["bond_idx"], np.int64).reshape(-1), minlength=A)
    return np.where((deg == 1) & (A > 2), 1.008, 12.0)


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def forces_nm(p, ff, pairs=None):
    """(F [B, A, 3], S [B, A], E [B], sums [B, 4]) at the positions p [B, A, 3] in nm, in p's float type: F = -dE / dp in kJ / (mol nm),
    S = 1 + the sum over the terms touching an atom of the norm of their contribution to it (float64), and the energy of the same
    terms, ((bond + angle) + torsion) + pair."""
    ft = p.dtype.type
    B, A = p.shape[:2]
    pairs = fn.pair_table(ff, A) if pairs is None else pairs
    F, S = np.zeros((B, A, 3), p.dtype), np.ones((B, A))
    sums = np.zeros((B, 4), p.dtype)

    def put(atoms, g):                                           # g [B, n, 3]: the force of each term on its atom `atoms` [n]
        np.add.at(F, (slice(None), atoms), g)                    # unbuffered: in table order
        np.add.at(S, (slice(None), atoms), np.nan_to_num(_norm(g.astype(np.float64)), nan=0.0, posinf=0.0))

    bi, bp = np.asarray(ff["bond_idx"], np.int64).reshape(-1, 2), np.asarray(ff["bond_par"], np.float64).reshape(-1, 2).astype(ft)
    ai, ap = np.asarray(ff["angle_idx"], np.int64).reshape(-1, 3), np.asarray(ff["angle_par"], np.float64).reshape(-1, 2).astype(ft)
    ti, tp = np.asarray(ff["torsion_idx"], np.int64).reshape(-1, 4), np.asarray(ff["torsion_par"], np.float64).reshape(-1, 3).astype(ft)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if len(bi):                                              # k (r - r0)^2 / 2: on slot 1 -k (r - r0) d / r, d = x1 - x0
            d = p[:, bi[:, 1]] - p[:, bi[:, 0]]
            r = _norm(d)
            dr = r - bp[:, 0]
            g = (-(bp[:, 1] * dr) / r)[..., None] * d
            put(bi[:, 1], g); put(bi[:, 0], -g)
            sums[:, 0] = (bp[:, 1] * dr * dr * ft(0.5)).sum(-1)
        if len(ai):                                              # k (theta - theta0)^2 / 2 through d theta / d cos = -1 / sin
            u, v = p[:, ai[:, 0]] - p[:, ai[:, 1]], p[:, ai[:, 2]] - p[:, ai[:, 1]]
            nu, nv = _norm(u), _norm(v)
            cs = np.clip((u * v).sum(-1) / (nu * nv), ft(-1), ft(1))
            dth = np.arccos(cs) - ap[:, 0]
            w = ap[:, 1] * dth / np.sqrt((ft(1) - cs) * (ft(1) + cs))
            gi = (w / nu)[..., None] * (v / nv[..., None] - cs[..., None] * (u / nu[..., None]))
            gk = (w / nv)[..., None] * (u / nu[..., None] - cs[..., None] * (v / nv[..., None]))
            put(ai[:, 0], gi); put(ai[:, 2], gk); put(ai[:, 1], -(gi + gk))
            sums[:, 1] = (ap[:, 1] * dth * dth * ft(0.5)).sum(-1)
        if len(ti):                                              # k (1 + cos(n phi - phase)): k n sin(n phi - phase) d phi / dx
            b1, b2, b3 = p[:, ti[:, 1]] - p[:, ti[:, 0]], p[:, ti[:, 2]] - p[:, ti[:, 1]], p[:, ti[:, 3]] - p[:, ti[:, 2]]
            m, n = np.cross(b1, b2), np.cross(b2, b3)
            l2 = (b2 * b2).sum(-1)
            l = np.sqrt(l2)
            phi = np.arctan2(l * (b1 * n).sum(-1), (m * n).sum(-1))
            arg = tp[:, 0] * phi - tp[:, 1]
            w = tp[:, 2] * tp[:, 0] * np.sin(arg)                # -dE / d phi
            d1 = (-l / (m * m).sum(-1))[..., None] * m           # d phi / d x1
            d4 = (l / (n * n).sum(-1))[..., None] * n            # d phi / d x4
            s12, s32 = ((b1 * b2).sum(-1) / l2)[..., None], ((b3 * b2).sum(-1) / l2)[..., None]
            d2 = -d1 - s12 * d1 + s32 * d4
            d3 = -d4 + s12 * d1 - s32 * d4
            for slot, dd in enumerate((d1, d2, d3, d4)):
                put(ti[:, slot], w[..., None] * dd)
            sums[:, 2] = (tp[:, 2] * (ft(1) + np.cos(arg))).sum(-1)
        ii, jj = np.triu_indices(A, 1)
        pr = np.asarray(pairs, np.float64).reshape(-1, 3)
        live = (pr[:, 0] != 0) | (pr[:, 2] != 0)
        ii, jj, pr = ii[live], jj[live], pr[live].astype(ft)
        if len(ii):                                              # 24 eps (2 s^2 - s) / r^2 + coulomb qq / r^3, times d = x_i - x_j, on i
            coulomb = ft(np.float64(ff.get("coulomb", fn.COULOMB)))
            d = p[:, ii] - p[:, jj]
            r2 = (d * d).sum(-1)
            r = np.sqrt(r2)
            qq, sigma, eps = pr[:, 0], pr[:, 1], pr[:, 2]
            q2 = (sigma / r) ** 2
            s6 = q2 * q2 * q2
            lj = np.where((eps > 0) & (sigma > 0), ft(24) * eps * s6 * (ft(2) * s6 - ft(1)) / r2, ft(0))
            cl = np.where(qq != 0, coulomb * qq / (r2 * r), ft(0))
            g = (lj + cl)[..., None] * d
            put(ii, g); put(jj, -g)
            sums[:, 3] = fn.pair_energy(r, qq, sigma, eps, coulomb).sum(-1)
    E = ((sums[:, 0] + sums[:, 1]) + sums[:, 2]) + sums[:, 3]
    return F, S, E, sums


def forces(x, to_nm, ff, pairs=None, T=None, ft=np.float64):
    """(F, S, E) of x [B, A, 3] fp32 at positions x * to_nm, as ti_obs_ff_forces states them: with T [B] every one divided by R T_b"""
    p = np.asarray(x, np.float32).astype(ft) * ft(np.float64(to_nm))
    F, S, E, _ = forces_nm(p, ff, pairs)
    if T is not None:
        rt = ft(fn.R_GAS) * np.asarray(T, np.float32).astype(ft)
        F, E, S = F / rt[:, None, None], E / rt, S / rt.astype(np.float64)[:, None]
    return F, S, E


def oracle_normal(seed, traj, step, comp):
    from oracle import oracle
    return np.float32(oracle.normal(int(seed), int(traj), int(step), int(comp)))


def draw_velocities(T, ids, masses, seed, step_offset, normal=oracle_normal, ft=np.float64):
    """[B, A, 3]: sqrt(R T_b / m_a) N(seed, id_b, step_offset, 3A + 3a + c)"""
    m = np.asarray(masses, np.float64).astype(ft)
    A = len(m)
    rt = ft(fn.R_GAS) * np.asarray(T, np.float32).astype(ft)
    xi = np.array([[normal(seed, i, step_offset, 3 * A + c) for c in range(3 * A)] for i in ids], np.float32).astype(ft).reshape(-1, A, 3)
    return np.sqrt(rt[:, None] / m[None, :])[..., None] * xi


def langevin(pos, vel, T, ids, ff, masses, dt, friction, n_steps, stride=0, step_offset=0, seed=0, to_nm=1.0, draw=False,
             normal=oracle_normal, ft=np.float64, pairs=None):
    """OpenMM's Langevin "middle" scheme as ti_obs_ff_langevin states it -> (pos, vel, frames fp32 [B, n_frames, A, 3], epot, ekin
    [B, n_frames]); the noise of global step s is normal(seed, id_b, s, 3a + c), promoted from fp32."""
    pos = np.array(pos, ft)
    B, A = pos.shape[:2]
    pairs = fn.pair_table(ff, A) if pairs is None else pairs
    m = np.asarray(masses, np.float64).astype(ft)[None, :, None]
    rt = (ft(fn.R_GAS) * np.asarray(T, np.float32).astype(ft))[:, None, None]
    vel = draw_velocities(T, ids, masses, seed, step_offset, normal, ft) if draw else np.array(vel, ft)
    dt, half = ft(np.float64(dt)), ft(np.float64(dt)) * ft(0.5)
    a = np.exp(-ft(np.float64(friction)) * dt)
    amp = np.sqrt((ft(1) - a * a) * rt / m)
    frames, epot, ekin = [], [], []
    F, _, E, _ = forces_nm(pos, ff, pairs)
    for s in range(n_steps):
        vel = vel + dt * F / m
        pos = pos + half * vel
        if friction > 0:
            xi = np.array([[normal(seed, i, step_offset + s, c) for c in range(3 * A)] for i in ids], np.float32).astype(ft).reshape(B, A, 3)
            vel = a * vel + amp * xi
        pos = pos + half * vel
        F, _, E, _ = forces_nm(pos, ff, pairs)
        if stride > 0 and (s + 1) % stride == 0:
            mean = np.zeros((B, 3), ft)
            for k in range(A):                                    # the atoms in order
                mean = mean + pos[:, k]
            frames.append(((pos - (mean / ft(A))[:, None]) / ft(np.float64(to_nm))).astype(np.float32))
            epot.append(E.copy())
            ekin.append((m * vel * vel * ft(0.5)).sum((1, 2)))
    nf = len(frames)
    stack = lambda v, shape, dtype: np.stack(v, axis=1) if nf else np.zeros(shape, dtype)
    return pos, vel, stack(frames, (B, 0, A, 3), np.float32), stack(epot, (B, 0), ft), stack(ekin, (B, 0), ft)


def energy_nm(p, ff, pairs=None):
    """E [B] of the positions p [B, A, 3] in nm, in p's float type, from the term energies of ff_numpy (fn.bond_energy, fn._angle,
    fn._torsion, fn.pair_energy) in fn.energies' order: fn.energies without the fp32 coordinates, for central differences"""
    ft = p.dtype.type
    A = p.shape[1]
    pairs = fn.pair_table(ff, A) if pairs is None else pairs
    bi, bp = np.asarray(ff["bond_idx"], np.int64).reshape(-1, 2), np.asarray(ff["bond_par"], np.float64).reshape(-1, 2).astype(ft)
    ai, ap = np.asarray(ff["angle_idx"], np.int64).reshape(-1, 3), np.asarray(ff["angle_par"], np.float64).reshape(-1, 2).astype(ft)
    ti, tp = np.asarray(ff["torsion_idx"], np.int64).reshape(-1, 4), np.asarray(ff["torsion_par"], np.float64).reshape(-1, 3).astype(ft)
    d = p[:, bi[:, 1]] - p[:, bi[:, 0]]
    e_bond = fn.bond_energy(_norm(d), bp[:, 0], bp[:, 1])
    e_angle = fn.angle_energy(fn._angle(p, ai[:, 0], ai[:, 1], ai[:, 2], ft), ap[:, 0], ap[:, 1])
    e_tors = fn.torsion_energy(fn._torsion(p, ti[:, 0], ti[:, 1], ti[:, 2], ti[:, 3]), tp[:, 0], tp[:, 1], tp[:, 2])
    ii, jj = np.triu_indices(A, 1)
    pr = np.asarray(pairs, np.float64).reshape(-1, 3)
    live = (pr[:, 0] != 0) | (pr[:, 2] != 0)
    ii, jj, pr = ii[live], jj[live], pr[live].astype(ft)
    d = p[:, jj] - p[:, ii]
    e_pair = fn.pair_energy(_norm(d), pr[:, 0], pr[:, 1], pr[:, 2], ft(np.float64(ff.get("coulomb", fn.COULOMB))))
    s = [np.asarray(e, ft).reshape(p.shape[0], -1).sum(-1) for e in (e_bond, e_angle, e_tors, e_pair)]
    return ((s[0] + s[1]) + s[2]) + s[3]
