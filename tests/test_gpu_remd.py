"""ti_obs_ff_remd on the GPU: every exchange decision re-derived exactly from the returned energies with the numpy restatement's rule
(tests/remd_numpy.py), a whole trajectory against the restatement where no decision is marginal (tests/test_remd_host.py checks
that on the CPU), the bitwise contract (repeat, host against device memory, ladders reversed, a ladder alone, chained, launch cut, no
attempt = ti_obs_ff_langevin), the physics of a diatomic ladder against quadrature, the failure path, the refusals, and
drivers.generate_md end to end with exchange_every on.

Mutations the physics test catches, MI355X: profiles/remd_mutations.txt."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from conftest import pkg
import ff_numpy as fn
import ff_forces_numpy as ffn
import remd_numpy as rn
from test_gpu_forcefield import engine, write_xml
from test_gpu_md import bits, same, species, with_md
from test_remd_host import TRAJ, TRAJ_EVERY, TRAJ_K, TRAJ_LADDERS, trajectory_case

pytestmark = pytest.mark.gpu

LD = np.longdouble


def ladders(name, K, L, big_ids=False):
    """L ladders of K rungs on the species' fixture geometries: T_k = 300 * 1.03^k (neighbouring rungs close enough that delta is
    of order 1), ids as test_gpu_md's, ladder ids small or beyond 32 bits"""
    eng, ff, m, x, to_nm = with_md(name)
    B = K * L
    pos = x[np.arange(B) % len(x)].astype(np.float64) * to_nm
    T = np.tile((300.0 * 1.03 ** np.arange(K)).astype(np.float32), L)
    ids = np.arange(B, dtype=np.int64) * 3 + 7
    lids = (np.array([2 ** 32 + 1, 2 ** 40 + 9, 2 ** 62 + 3, -2, 7], np.int64)[np.arange(L) % 5] + np.arange(L) // 5) if big_ids \
        else np.arange(L, dtype=np.int64) + 5
    return eng, ff, m, pos, T, ids, lids, to_nm


# ---- every decision, exactly -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,L,big", [("A2", 2, 1, False), ("A2", 3, 1, False), ("A2", 64, 1, False), ("A2", 64, 3, False),
                                          ("A4", 3, 5, False), ("A9", 8, 3, True)])
def test_every_decision_is_the_rule_applied_to_the_returned_energies(name, K, L, big):
    """stride == exchange_every: out_epot holds E_k of every row right before every attempt, bit for bit what the kernel decided on.
    The restatement's rule on those energies, T, seed and the ladder ids must give out_walker and out_counts, every attempt of every
    pair.  K = 3: rung 0 or 2 sits out in turn; K = 64: the fourth counter word goes up to DOMAIN + 15; A4, 5 ladders of one pair
    each: the pairs straddle workgroups of four waves; A9: ladder ids beyond 32 bits."""
    eng, ff, m, pos, T, ids, lids, to_nm = ladders(name, K, L, big)
    every, n_att, seed, off = 2, 10, 2 ** 40 + 11, 6
    p, v, fr, ep, ek, w, hist, cnt = eng.remd(pos, None, T, K, every, 1e-4, 1.0, every * n_att, stride=every, step_offset=off, seed=seed, ids=ids,
                                             ladder_ids=lids, to_nm=to_nm, draw_velocities=True)
    assert hist.shape == (n_att, K * L) and hist.dtype == np.int32 and cnt.shape == (L, K - 1, 2) and cnt.dtype == np.int64 and ep.shape == (K * L, n_att)
    assert np.isfinite(ep).all() and np.isfinite(p).all()
    attempts = [off // every + 1 + j for j in range(n_att)]
    want_hist, want_cnt, accepted, margins = rn.replay(ep, T, K, seed, lids, attempts)
    n_acc = sum(accepted.values())
    print(f"{name} K = {K}, {L} ladders: {len(accepted)} decisions, {n_acc} accepted, smallest |logu - delta| = {margins.min():.2e}")
    assert len(accepted) == sum(len(rn.pairs(n, K)) for n in attempts) * L
    np.testing.assert_array_equal(hist, want_hist)
    np.testing.assert_array_equal(cnt, want_cnt)
    np.testing.assert_array_equal(w, want_hist[-1])
    assert (np.sort(hist.reshape(n_att, L, K), axis=2) == np.arange(K)).all()                    # a permutation within each ladder
    if K * L >= 15:                                              # enough decisions that both outcomes occur
        assert 0 < n_acc < len(accepted)


# ---- a trajectory against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A4", "A9"])
def test_trajectory_parity(name):
    """16 steps, an attempt every 4, three ladders of three rungs: accept / reject identical and the state within 100 d64 (d64: the
    restatement's own fp64 error against np.longdouble on the same run, tests/test_gpu_md.py's bar).  Valid because no decision of
    the run is marginal, asserted here as tests/test_remd_host.py asserts it without a GPU."""
    if np.finfo(LD).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here: d64 cannot be formed")
    (ff, m, pos, T, ids, lids, to_nm), r64 = trajectory_case(name)
    _, r80 = trajectory_case(name, LD)
    assert r64[8].min() > 1e-6 and 0 < r64[7][..., 1].sum() < r64[7][..., 0].sum() and len(r64[8]) == TRAJ_LADDERS * 4
    assert np.array_equal(r64[6], r80[6]) and np.array_equal(r64[7], r80[7])                      # the wider run decides the same
    d64 = float(max(np.abs(r64[0] - r80[0]).max(), np.abs(r64[1] - r80[1]).max()))
    eng = with_md(name)[0]
    p, v, fr, ep, ek, w, hist, cnt = eng.remd(pos, None, T, TRAJ_K, TRAJ_EVERY, TRAJ["dt"], TRAJ["friction"], TRAJ["n_steps"], stride=TRAJ["stride"],
                                             seed=TRAJ["seed"], ids=ids, ladder_ids=lids, to_nm=to_nm, draw_velocities=True)
    np.testing.assert_array_equal(hist, r64[6])
    np.testing.assert_array_equal(cnt, r64[7])
    np.testing.assert_array_equal(w, r64[5])
    dp, dv = float(np.abs(p - r64[0]).max()), float(np.abs(v - r64[1]).max())
    print(f"{name}: d64 = {d64:.3e}; |dpos| = {dp:.3e}, |dvel| = {dv:.3e} ({max(dp, dv) / d64:.2f} d64; bar 100); {cnt[..., 1].sum()} of {cnt[..., 0].sum()} accepted")
    assert max(dp, dv) <= 100 * d64, (name, dp, dv, d64)
    tol_f = 100 * d64 / to_nm + np.spacing(np.abs(r64[2]))
    assert (np.abs(fr.astype(np.float64) - r64[2].astype(np.float64)) <= tol_f).all()


# ---- bits ------------------------------------------------------------------------------------------------------------------------
def go(eng, pos, vel, T, ids, lids, to_nm, walker=None, **over):
    kw = dict(dict(TRAJ, every=TRAJ_EVERY), **over)
    return eng.remd(pos, vel, T, TRAJ_K, kw["every"], kw["dt"], kw["friction"], kw["n_steps"], stride=kw["stride"], seed=kw["seed"], ids=ids,
                    ladder_ids=lids, walker=walker, to_nm=to_nm, draw_velocities=vel is None, step_offset=kw.get("step_offset", 0),
                    steps_per_launch=kw.get("steps_per_launch", 0))


def test_bitwise_contract():
    torch = pytest.importorskip("torch")
    (ff, m, pos, T, ids, lids, to_nm), _ = trajectory_case("A9")
    eng = with_md("A9")[0]
    K, L = TRAJ_K, TRAJ_LADDERS
    ref = go(eng, pos, None, T, ids, lids, to_nm)
    assert all(np.isfinite(a).all() for a in ref[:5]) and 0 < ref[7][..., 1].sum() < ref[7][..., 0].sum()
    same(go(eng, pos, None, T, ids, lids, to_nm), ref)                                           # the same call twice
    dev = go(eng, torch.from_numpy(pos).cuda(), None, torch.from_numpy(T).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(lids).cuda(), to_nm)
    assert all(a.is_cuda for a in dev) and dev[5].dtype == dev[6].dtype == torch.int32 and dev[7].dtype == torch.int64
    same([a.cpu().numpy() for a in dev], ref)                                                    # device memory
    # the ladders in reverse order in the batch, each with its ids and its ladder id
    lad = lambda a, axis=0: a.reshape(a.shape[:axis] + (L, K) + a.shape[axis + 1:])
    flip = lambda a: lad(a)[::-1].reshape(a.shape).copy()
    rev = go(eng, flip(pos), None, flip(T), flip(ids), lids[::-1].copy(), to_nm)
    same([flip(a) for a in rev[:6]], ref[:6])
    np.testing.assert_array_equal(lad(rev[6], 1)[:, ::-1].reshape(rev[6].shape), ref[6])
    np.testing.assert_array_equal(rev[7][::-1], ref[7])
    for l in (0, 2):                                                                             # a ladder alone
        rows = slice(l * K, (l + 1) * K)
        one = go(eng, pos[rows], None, T[rows], ids[rows], lids[l:l + 1], to_nm)
        same(one[:6], [a[rows] for a in ref[:6]])
        np.testing.assert_array_equal(one[6], ref[6][:, rows])
        np.testing.assert_array_equal(one[7], ref[7][l:l + 1])
    # 16 steps against 5 + 5 + 5 + 1 chained with step_offset, the labels carried over; a frame after every step
    p0, v0 = go(eng, pos, None, T, ids, lids, to_nm, n_steps=0, stride=0)[:2]
    whole = go(eng, p0, v0, T, ids, lids, to_nm, stride=1, step_offset=102)
    assert len(whole[6]) == 4                                                                    # attempts behind steps 104, 108, 112, 116
    parts, state, walker, at = [], (p0, v0), None, 102
    for n in (5, 5, 5, 1):
        parts.append(go(eng, state[0], state[1], T, ids, lids, to_nm, walker=walker, n_steps=n, stride=1, step_offset=at))
        state, walker, at = parts[-1][:2], parts[-1][5], at + n
    assert [len(q[6]) for q in parts] == [1, 2, 1, 0]
    same([parts[-1][0], parts[-1][1], parts[-1][5]], [whole[0], whole[1], whole[5]])
    same([np.concatenate([q[i] for q in parts], axis=1) for i in (2, 3, 4)], whole[2:5])
    np.testing.assert_array_equal(np.concatenate([q[6] for q in parts]), whole[6])
    np.testing.assert_array_equal(sum(q[7] for q in parts), whole[7])
    same(go(eng, pos, None, T, ids, lids, to_nm, steps_per_launch=3), ref)                       # the launch cut
    same(go(eng, pos, None, T, ids, lids, to_nm, steps_per_launch=1024), ref)
    # no attempt falls into the run: ti_obs_ff_langevin bit for bit in every output
    none = go(eng, pos, None, T, ids, lids, to_nm, every=17)
    plain = eng.langevin(pos, None, T, TRAJ["dt"], TRAJ["friction"], TRAJ["n_steps"], stride=TRAJ["stride"], seed=TRAJ["seed"], ids=ids, to_nm=to_nm,
                         draw_velocities=True)
    same(none[:5], plain)
    assert none[5].tolist() == list(range(K)) * L and none[6].shape == (0, K * L) and not none[7].any()
    assert not all(np.array_equal(a, b) for a, b in zip(ref[:2], plain[:2]))                      # and the exchanges do change the run


# ---- physics ---------------------------------------------------------------------------------------------------------------------
def test_diatomic_ladder_against_quadrature():
    """A2 with masses 12: 128 ladders of 300 / 1000 K, dt = 1 fs, friction 0.1 / ps and an attempt every 7 steps (the pair is tried at
    every second one), so velocities exchanged without the rescale would not have relaxed before the next frame; 2000 steps, then
    20000 with a frame every 20.  The bond lengths start from the exact densities (inverse CDF on the quadrature grid; at this
    friction a start at r0 would take 10 ps to gain its potential energy).  Per rung <r>, <(r - r0)^2> against the quadrature of
    r^2 exp(-k (r - r0)^2 / (2 R T)) and <ekin> against 3 R T, and the acceptance fraction against the two-dimensional quadrature of
    min(1, exp(delta)) over the two densities: each within 5 standard errors over the 128 ladder means
    (test_bond_length_distribution_of_a_diatomic's bar).  A flipped sign of delta, a missing velocity rescale, and a rescale of the
    stored velocity as it is (half a kick behind the positions) each fail it: profiles/remd_mutations.txt."""
    ti = pkg()
    eng, ff, m, x, to_nm = with_md("A2", masses=np.array([12.0, 12.0]))
    r0, k = ff["bond_par"][0]
    L, temps = 128, np.float32([300.0, 1000.0])
    grid = np.linspace(max(r0 - 0.08, 1e-4), r0 + 0.08, 200001)
    dens = [grid ** 2 * np.exp(-k * (grid - r0) ** 2 / (2 * fn.R_GAS * float(t))) for t in temps]
    dens = [w / w.sum() for w in dens]
    rs = np.random.RandomState(7)
    start = np.zeros((L, 2, 2, 3))
    for j, w in enumerate(dens):
        start[:, j, 1, 0] = np.interp(rs.random_sample(L), np.cumsum(w), grid)
    smp = ti.md.ReplicaExchangeSampler(eng, ti.forcefield.ForceField(**ff, masses=[12.0, 12.0]), to_nm, 1e-3, 0.1, seed=2024, exchange_every=7)
    smp.start(start.reshape(2 * L, 2, 3) / to_nm, temps, L).equilibrate(2000)
    frames, epot, ekin = smp.sample(1000, 20)
    assert frames.shape == (2 * L, 1000, 2, 3) and smp.step == 22000 and smp.walkers.shape == (22000 // 7, L, 2)
    assert (smp.counts[:, 0, 0] == 22000 // 14).all()                                            # the pair is tried at the even attempts
    r = (np.linalg.norm((frames[:, :, 1] - frames[:, :, 0]).astype(np.float64), axis=-1) * to_nm).reshape(L, 2, 1000)
    kin = ekin.reshape(L, 2, 1000)
    worst = 0.0
    for j, temp in enumerate(temps):
        mean_q, var_q = (dens[j] * grid).sum(), (dens[j] * (grid - r0) ** 2).sum()
        for what, per_ladder, want in (("<r>", r[:, j].mean(axis=1), mean_q), ("<(r - r0)^2>", ((r[:, j] - r0) ** 2).mean(axis=1), var_q),
                                       ("<ekin>", kin[:, j].mean(axis=1), 3 * fn.R_GAS * float(temp))):
            est, se = per_ladder.mean(), per_ladder.std(ddof=1) / np.sqrt(L)
            z = (est - want) / se
            worst = max(worst, abs(z))
            print(f"T = {temp:.0f} K {what}: {est:.6e} against {want:.6e}, z = {z:+.2f}, relative standard error {se / want:.2e}")
            assert abs(z) <= 5.0, (temp, what, z)
    # the acceptance: E = k (r - r0)^2 / 2 of the two rungs' bond lengths, on a coarser grid (the integrand is smooth)
    g = grid[::100]
    w0, w1 = dens[0][::100] / dens[0][::100].sum(), dens[1][::100] / dens[1][::100].sum()
    E = k * (g - r0) ** 2 / 2
    delta = (1 / (fn.R_GAS * 300.0) - 1 / (fn.R_GAS * 1000.0)) * (E[:, None] - E[None, :])
    acc_q = float((w0[:, None] * w1[None, :] * np.minimum(1.0, np.exp(delta))).sum())
    per_ladder = smp.counts[:, 0, 1] / smp.counts[:, 0, 0]
    est, se = per_ladder.mean(), per_ladder.std(ddof=1) / np.sqrt(L)
    z = (est - acc_q) / se
    trips = ti.md.round_trips(smp.walkers)
    print(f"acceptance: {est:.5f} against {acc_q:.5f}, z = {z:+.2f}, standard error {se:.1e}; round trips per ladder {trips.mean():.1f}; worst |z| above {worst:.2f}")
    assert abs(z) <= 5.0, z
    np.testing.assert_allclose(smp.acceptance, [est], rtol=1e-12)
    assert (trips > 0).all()


# ---- failure and refusals --------------------------------------------------------------------------------------------------------
def raw(eng, pos, vel, T, walker, B=None, mem=0, ids=None, lids=None, to_nm=1.0, r=(3, 0, 2), n_att=2, **d):
    """ti_obs_ff_remd through ctypes on host memory with poisoned outputs -> (rc, frames, epot, ekin, out_walker, out_counts)"""
    ti = pkg()
    kw = dict(dt=5e-4, friction=1.0, n_steps=4, stride=2, step_offset=0, traj_offset=0, seed=1, draw_velocities=0, steps_per_launch=0)
    kw.update({k: v for k, v in d.items() if k in kw})
    desc = ti._lib.MdDesc(*(kw[k] for k in ("dt", "friction", "n_steps", "stride", "step_offset", "traj_offset", "seed", "draw_velocities",
                                           "steps_per_launch")))
    rd = None if r is None else ti._lib.RemdDesc(*r)
    n, A = (6, 9) if pos is None else pos.shape[:2]
    fr, ep, ek = np.full((n, 2, A, 3), -7.0, np.float32), np.full((n, 2), -7.0), np.full((n, 2), -7.0)
    hist, cnt = np.full((n_att, n), -7, np.int32), np.full((n, 2), -7, np.int64)                  # counts: roomy for every K tried
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = ti._lib.lib().ti_obs_ff_remd(eng.h, C.byref(desc) if d.get("desc", 1) else None, None if rd is None else C.byref(rd), ptr(pos), ptr(vel),
                                      ptr(T), ptr(ids), ptr(lids), n if B is None else B, to_nm, ptr(walker), ptr(fr), ptr(ep), ptr(ek), ptr(hist),
                                      ptr(cnt), mem)
    return rc, fr, ep, ek, hist, cnt


def remd_case():
    eng, ff, m, x, to_nm = with_md("A9")
    pos = x[:6].astype(np.float64) * to_nm
    T = np.tile(np.float32([300.0, 310.0, 320.0]), 2)
    return eng, ff, m, pos, T, np.arange(6, dtype=np.int64) * 3 + 7


def test_a_blown_up_replica_is_named_and_the_state_and_labels_are_left_alone():
    """test_gpu_md.py's collision in row 3 (rung 0 of ladder 1) with an attempt after every step: TI_E_NAN names the replica, pos, vel
    and walker keep their bits, a host call copies nothing back, and the handle goes on working"""
    ti = pkg()
    eng, ff, m, pos, T, ids = remd_case()
    tab = fn.pair_table(ff, 9)
    deg = np.bincount(np.asarray(ff["bond_idx"]).reshape(-1), minlength=9)
    i, j = next((i, j) for i in range(9) for j in range(9) if i != j and deg[i] >= 2 and tab[fn.pair_row(min(i, j), max(i, j), 9), 2] > 0)
    bad = pos.copy()
    bad[3, j] = bad[3, i] + np.array([1e-4, 0.0, 0.0])
    vel, walker = np.zeros_like(bad), np.int32([2, 1, 0, 1, 0, 2])
    p_in, w_in = bad.copy(), walker.copy()
    rc, fr, ep, ek, hist, cnt = raw(eng, bad, vel, T, walker, dt=2e-3, friction=0.0, n_steps=9, stride=5, r=(3, 0, 1), n_att=9)
    assert rc == ti._lib.TI_E_NAN and "replica 3" in ti._lib.last_error(), ti._lib.last_error()
    np.testing.assert_array_equal(bits(bad), bits(p_in))
    assert (vel == 0).all() and np.array_equal(walker, w_in)
    assert (fr == -7.0).all() and (ep == -7.0).all() and (ek == -7.0).all() and (hist == -7).all() and (cnt == -7).all()
    with pytest.raises(ti._lib.TiError, match="replica 3"):
        eng.remd(bad, vel, T, 3, 1, 2e-3, 0.0, 9, stride=5)
    rc, fr, ep, ek, hist, cnt = raw(eng, pos.copy(), np.zeros_like(pos), T, walker)
    assert rc == 0 and np.isfinite(ep).all() and sorted(walker[:3]) == [0, 1, 2] and (hist >= 0).all() and cnt[:4].sum() > 0


def test_refusals_write_nothing():
    torch = pytest.importorskip("torch")
    ti = pkg()
    ARG, UNS = ti._lib.TI_E_ARG, ti._lib.TI_E_UNSUPPORTED
    eng, ff, m, pos, T, ids = remd_case()
    vel, walker = np.zeros_like(pos), np.int32([0, 1, 2, 0, 1, 2])
    p_in = pos.copy()

    def refused(code, out, what, named=None):
        rc, fr, ep, ek, hist, cnt = out
        assert rc == code and ti._lib.last_error(), what
        assert named is None or named in ti._lib.last_error(), (what, ti._lib.last_error())
        assert (fr == -7.0).all() and (ep == -7.0).all() and (ek == -7.0).all() and (hist == -7).all() and (cnt == -7).all(), what
        np.testing.assert_array_equal(bits(pos), bits(p_in), err_msg=what)
        assert (vel == 0).all() and walker.tolist() == [0, 1, 2, 0, 1, 2], what

    # ti_obs_ff_langevin's refusals, in its order and before the new ones: each with a bad remd descriptor as well
    for r in ((3, 0, 2), None, (1, 0, 2)):
        refused(ARG, raw(eng, pos, vel, T, walker, desc=0, r=r), "NULL desc", "NULL desc")
        refused(ARG, raw(eng, None, vel, T, walker, r=r), "NULL pos", "NULL desc, pos or T")
        refused(ARG, raw(eng, pos, None, T, walker, r=r), "NULL vel without draw_velocities", "vel is NULL")
        refused(ARG, raw(eng, pos, vel, T, walker, dt=0.0, r=r), "dt = 0", "dt")
        refused(ARG, raw(eng, pos, vel, T, walker, friction=-1.0, r=r), "friction < 0", "friction")
        refused(ARG, raw(eng, pos, vel, T, walker, n_steps=-1, r=r), "n_steps < 0", "negative")
        refused(ARG, raw(eng, pos, vel, T, walker, B=0, r=r), "B < 1", "B < 1")
        refused(ARG, raw(eng, pos, vel, T, walker, mem=7, r=r), "unknown mem", "mem")
        refused(ARG, raw(eng, pos, vel, T, walker, to_nm=0.0, r=r), "to_nm = 0", "to_nm")
    # the new ones
    refused(ARG, raw(eng, pos, vel, T, walker, r=None), "NULL remd desc", "remd desc")
    for K in (1, 0, -3, 65):
        refused(ARG, raw(eng, pos, vel, T, walker, r=(K, 0, 2)), f"n_rungs = {K}", "n_rungs")
    refused(ARG, raw(eng, pos, vel, T, walker, r=(4, 0, 2)), "B % n_rungs != 0", "multiple")
    refused(ARG, raw(eng, pos, vel, T, walker, B=5), "B % n_rungs != 0", "multiple")
    for every in (0, -1):
        refused(ARG, raw(eng, pos, vel, T, walker, r=(3, 0, every)), f"exchange_every = {every}", "exchange_every")
    refused(ARG, raw(eng, pos, vel, T, walker, r=(3, 1, 2)), "reserved != 0", "reserved")
    for value, at in ((-1, 4), (3, 1)):
        wb = walker.copy()
        wb[at] = value
        out = raw(eng, pos, vel, T, wb, r=(3, 0, 2))
        refused(ARG, out, f"walker[{at}] = {value}", f"index {at}")
        assert wb[at] == value
    # found on the device: a bad temperature as ti_obs_ff_langevin finds it, a bad label in device memory, the temperature first
    Tb = T.copy()
    Tb[2], Tb[4] = np.nan, 0.0
    refused(ARG, raw(eng, pos, vel, Tb, walker), "T = nan", "T must be finite and > 0: index 2")
    dev = lambda a: torch.from_numpy(a).cuda()
    for Tin, wv, named in ((T, [0, 1, 2, 0, 3, 2], "walker must lie in 0 .. n_rungs - 1: index 4"), (T, [0, -1, 2, 0, 3, 2], "index 1"),
                           (Tb, [0, 1, 2, 0, 3, 2], "T must be finite and > 0: index 2")):
        with pytest.raises(ti._lib.TiError, match=named) as err:
            eng.remd(dev(pos), dev(vel), dev(Tin), 3, 2, 5e-4, 1.0, 4, stride=2, walker=dev(np.int32(wv)))
        assert err.value.code == ARG
    ok = eng.remd(dev(pos), dev(vel), dev(T), 3, 2, 5e-4, 1.0, 4, stride=2, walker=dev(walker))      # the handle goes on working
    assert torch.isfinite(ok[0]).all() and sorted(ok[5][:3].tolist()) == [0, 1, 2]
    adw = ti.observables._service_engine(0)
    refused(ARG, raw(adw, pos, vel, T, walker), "an adw handle", "painn handle")
    eng.set_molecules(np.full(6, 9, np.int32))
    try:
        refused(UNS, raw(eng, pos, vel, T, walker), "ti_painn_set_molecules in force")
    finally:
        eng.set_molecules(None)
    eng.set_forcefield(ti.forcefield.ForceField(**ff))                                           # a force field without masses
    refused(ARG, raw(eng, pos, vel, T, walker), "no masses", "masses")
    with pytest.raises(ValueError, match="masses"):
        eng.remd(pos, vel, T, 3, 2, 5e-4, 1.0, 4)
    eng.set_forcefield(None)
    refused(ARG, raw(eng, pos, vel, T, walker), "no force field", "force field")


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_generate_md_end_to_end_with_exchange(tmp_path):
    ti = pkg()
    ff, m, x, to_nm = species("A4")
    write_xml(ff, tmp_path / "ff.xml")
    text = (tmp_path / "ff.xml").read_text()
    for a in range(4):                                                                           # the species' masses in place of the writer's 1
        text = text.replace('<Particle mass="1"/>', f'<Particle mass="{float(m[a])!r}"/>', 1)
    (tmp_path / "ff.xml").write_text(text)
    np.save(tmp_path / "x0.npy", x[:3].astype(np.float64))

    def generate(sub, **over):
        cfg = types.SimpleNamespace(forcefield=str(tmp_path / "ff.xml"), x0=str(tmp_path / "x0.npy"), to_nm=to_nm, temperatures=[1000, 300, 400],
                                    n_replicas=4, dt=5e-4, friction=1.0, n_equil=10, n_frames=8, stride=2, seed=3,
                                    splits={"train": 0.5, "val": 0.25, "test": 0.25}, traj_path=str(tmp_path / sub), traj_filename="mol.npy", **over)
        paths = ti.drivers.generate_md(cfg, engine(4))
        with np.load(os.path.join(cfg.traj_path, "md_log.npz")) as z:
            return {s: np.load(p) for s, p in paths.items()}, {k: z[k] for k in z.files}

    files, log = generate("on", exchange_every=3)
    for split, n in (("train", 2), ("val", 1), ("test", 1)):
        a = files[split]
        assert a.shape == (8, n * 8, 4, 3) and a.dtype == np.float32 and np.isnan(a[2:7]).all() and np.isfinite(a[[0, 1, 7]]).all()
        assert np.abs(a[[0, 1, 7]].astype(np.float64).mean(axis=2)).max() <= 2e-7 * np.abs(a[[0, 1, 7]]).max()
    assert int(log["exchange_every"]) == 3 and log["accept_counts"].shape == (4, 2, 2) and log["round_trips"].shape == (4,)
    assert log["epot"].shape == (3, 4, 8) and np.isfinite(log["epot"]).all() and log["temperatures"].tolist() == [1000, 300, 400]
    # 26 steps: attempts 1 .. 8; the pair (300, 400) at the even ones, (400, 1000) at the odd ones
    assert log["accept_counts"][:, :, 0].tolist() == [[4, 4]] * 4
    assert (log["accept_counts"][..., 1] >= 0).all() and (log["accept_counts"][..., 1] <= 4).all() and (log["round_trips"] >= 0).all()
    # the key off: today's files and log, and a run into which no attempt falls writes the same files through the ladder path
    off, log_off = generate("off")
    zero, log_zero = generate("zero", exchange_every=0)
    far, log_far = generate("far", exchange_every=1000)
    assert not {"exchange_every", "accept_counts", "round_trips"} & (set(log_off) | set(log_zero)) and int(log_far["exchange_every"]) == 1000
    for other, other_log in ((zero, log_zero), (far, log_far)):
        for split in off:
            np.testing.assert_array_equal(bits(off[split]), bits(other[split]))
        np.testing.assert_array_equal(bits(log_off["epot"]), bits(other_log["epot"]))
        np.testing.assert_array_equal(bits(log_off["ekin"]), bits(other_log["ekin"]))
    assert not log_far["accept_counts"].any() and any(not np.array_equal(bits(off[s]), bits(files[s])) for s in off)
