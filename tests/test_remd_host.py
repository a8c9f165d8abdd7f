"""Replica exchange on the host: the C ABI's declaration, listing and export, the refusals that need no device, the numpy restatement
(tests/remd_numpy.py) on hand-made cases -- pairing, counter words, the uniform, the restated logf against the host libm, the
Metropolis rule, the velocity rescale --, md.round_trips, the fixture condition the GPU trajectory test relies on, and
drivers.generate_md's exchange_every key against a stub engine.  No GPU."""
import ctypes as C
import ctypes.util
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
import ff_numpy as fn
import ff_forces_numpy as ffn
import remd_numpy as rn
import vloss_numpy as vn
from test_ff_forces_host import StubEngine, fixtures, md_config, numpy_normal

LD = np.longdouble


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_declared_listed_and_exported():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    L = ti._lib.lib()
    assert re.search(r"\bint ti_obs_ff_remd\(ti_handle\* h, const ti_md_desc\* d, const ti_remd_desc\* r, ", hdr)
    assert "ti_obs_ff_remd" in ti._lib.ABI_SYMBOLS and hasattr(L, "ti_obs_ff_remd")
    assert "obs_ff_remd_kernels.hip" in ti.build.SOURCES and "ff_stage.hpp" in ti.build.HEADERS
    assert L.ti_version() == 5 and "#define TI_ABI_VERSION 5" in hdr
    assert "#define TI_REMD_MAX_RUNGS 64" in hdr and "#define TI_REMD_DOMAIN 0x52454D44u" in hdr
    assert (ti._lib.REMD_MAX_RUNGS, ti._lib.REMD_DOMAIN) == (rn.REMD_MAX_RUNGS, rn.REMD_DOMAIN) == (64, 0x52454D44)
    assert C.sizeof(ti._lib.RemdDesc) == 16 and ti._lib.RemdDesc.exchange_every.offset == 8
    assert rn.REMD_DOMAIN > 64 and rn.REMD_DOMAIN + (rn.REMD_MAX_RUNGS - 1 >> 2) < 2 ** 32    # beyond every noise / velocity draw's word


def test_refusals_before_the_device():
    """without a device there is no handle: the first refusal of the order, and the Python layer's own (an engine object without a
    handle stands in).  The refusals behind a live handle are in tests/test_gpu_remd.py."""
    ti = pkg()
    L = ti._lib.lib()
    d, r = ti._lib.MdDesc(1e-3, 1.0, 4, 0, 0, 0, 0, 0, 0), ti._lib.RemdDesc(2, 0, 2)
    assert L.ti_obs_ff_remd(None, C.byref(d), C.byref(r), None, None, None, None, None, 2, 1.0, None, None, None, None, None, None, 0) == ti._lib.TI_E_ARG
    assert ti._lib.last_error() == "not a painn handle"
    eng = object.__new__(ti.engine.PainnEngine)
    eng.A = 5
    pos = np.zeros((4, 5, 3))
    with pytest.raises(ValueError, match="force field"):
        eng.remd(pos, pos, 300.0, 2, 2, 1e-3, 1.0, 1)
    eng._ff_set, eng._ff_constraints, eng._ff_masses = True, True, True
    with pytest.raises(ValueError, match="constraints"):
        eng.remd(pos, pos, 300.0, 2, 2, 1e-3, 1.0, 1)
    eng._ff_constraints, eng._ff_masses = False, False
    with pytest.raises(ValueError, match="masses"):
        eng.remd(pos, pos, 300.0, 2, 2, 1e-3, 1.0, 1)
    eng._ff_masses = True
    for K, every in ((3, 2), (1, 2), (2, 0)):
        with pytest.raises(ValueError, match="n_rungs"):
            eng.remd(pos, pos, 300.0, K, every, 1e-3, 1.0, 1)


# ---- 2. the restatement on hand-made cases -----------------------------------------------------------------------------------------
def test_pairing():
    assert rn.pairs(0, 2) == [0] and rn.pairs(1, 2) == [] and rn.pairs(2, 3) == [0] and rn.pairs(3, 3) == [1]
    assert rn.pairs(4, 8) == [0, 2, 4, 6] and rn.pairs(5, 8) == [1, 3, 5] and rn.pairs(7, 64)[-1] == 61 and rn.pairs(6, 64)[-1] == 62
    for K in (2, 3, 8, 64):                                      # two consecutive attempts try every neighbouring pair once
        assert sorted(rn.pairs(10, K) + rn.pairs(11, K)) == list(range(K - 1))


def test_counter_words_uniform_and_logf():
    lid = 2 ** 40 + 9
    assert rn.counter(lid, 7, 5) == [9, 2 ** 8, 7, 0x52454D44 + 1] and rn.counter(-2, 2 ** 32 + 3, 63) == [0xFFFFFFFE, 0xFFFFFFFF, 3, 0x52454D44 + 15]
    # the draw by hand: pair (5, 6) reads word 1 of the block with fourth word DOMAIN + 1
    seed = 2 ** 40 + 11
    o = vn.philox4x32_10(np.asarray([[9, 2 ** 8, 7, 0x52454D45]], np.uint64), (11, 2 ** 8))
    u = (np.float32(int(o[0, 1]) >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert 0 < u < 1 and rn.uniform24(o[0, 1]) == u
    assert rn.draw_logu(seed, lid, 7, 5) == float(rn.host_logf(u)) < 0
    assert rn.draw_logu(seed, lid, 7, 5) != rn.draw_logu(seed, lid, 7, 4) != rn.draw_logu(seed, lid, 8, 4)
    assert rn.uniform24(0) == np.float32(2.0 ** -25) and rn.uniform24(0xFFFFFFFF) == np.float32(1 - 2.0 ** -25)
    # the restated logf is the host libm's on the uniforms of the draw: the ends, and 200000 words
    name = ctypes.util.find_library("m")
    if not name:
        pytest.skip("no libm to compare with")
    libm = C.CDLL(name)
    libm.logf.restype, libm.logf.argtypes = C.c_float, [C.c_float]
    words = np.concatenate([np.uint32([0, 255, 256, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF]), np.random.RandomState(0).randint(0, 2 ** 32, 200000, np.uint64).astype(np.uint32)])
    us = rn.uniform24(words)
    want = np.array([libm.logf(float(v)) for v in us], np.float32)
    np.testing.assert_array_equal(rn.host_logf(us).view(np.uint32), want.view(np.uint32))


def test_metropolis_rule_on_a_hand_made_ladder():
    T = np.float32([300.0, 600.0, 1200.0])
    b = 1.0 / (fn.R_GAS * T.astype(np.float64))
    # the cold rung above the hot one in energy: always accepted (delta >= 0); the other way round by exp(delta)
    d = rn.decide([10.0, 0.0, 5.0], T, 3, 0, 0)
    assert list(d) == [0] and d[0][0] is True and d[0][1] == (b[0] - b[1]) * 10.0 > 0
    d = rn.decide([0.0, 1000.0, 5.0], T, 3, 0, 0)
    assert d[0][0] is False and d[0][1] == (b[0] - b[1]) * -1000.0 < d[0][2] < 0
    d = rn.decide([0.0, 1000.0, 5.0], T, 3, 0, 1)                # the odd attempt pairs (1, 2)
    assert list(d) == [1] and d[1][0] is True
    d = rn.decide([0.0, 1e-9, 5.0], T, 3, 0, 0)                  # delta just below 0: logu < delta decides
    assert d[0][1] < 0 and d[0][0] == (d[0][2] < d[0][1])
    assert rn.decide([np.nan, 0.0, 5.0], T, 3, 0, 0)[0][0] is False and rn.decide([np.inf, 0.0, 5.0], T, 3, 0, 0)[0][0] is False
    assert rn.decide([10.0, 0.0, 5.0], T, 3, 0, 0, dead=[False, True, False])[0][0] is False
    # the long-run acceptance of a fixed delta is exp(delta)
    delta = -0.7
    E = [0.0, -delta / (b[0] - b[1]), 0.0]
    acc = np.mean([rn.decide(E, T, 5, l, 2 * n)[0][0] for l in range(40) for n in range(100)])
    assert abs(acc - np.exp(delta)) < 5 * np.sqrt(np.exp(delta) * (1 - np.exp(delta)) / 4000)


def test_replay_follows_walkers_and_counts():
    T = np.tile(np.float32([300.0, 600.0, 1200.0]), 2)
    epot = np.array([[10.0, 0.0], [0.0, 1000.0], [5.0, 0.0], [0.0, 0.0], [1000.0, 1000.0], [0.0, 0.0]])      # [B = 6, two attempts]
    hist, counts, accepted, margins = rn.replay(epot, T, 3, 3, None, [2, 3])
    assert accepted == {(0, 0, 0): True, (0, 1, 0): False, (1, 0, 1): True, (1, 1, 1): True}
    assert hist.tolist() == [[1, 0, 2, 0, 1, 2], [1, 2, 0, 0, 2, 1]] and len(margins) == 4
    assert counts.tolist() == [[[1, 1], [1, 1]], [[1, 0], [1, 1]]]


def test_the_restated_exchange_swaps_and_rescales():
    """A4, one ladder of three rungs, one step per attempt, the energies arranged by the geometries: after an accepted exchange the
    rows hold each other's positions and the velocities times sqrt(T_new / T_old); a run in which no attempt falls is
    ff_forces_numpy.langevin"""
    ff, x, to_nm = next((ff, x, to_nm) for n, ff, x, to_nm in fixtures() if n == "A4")
    m = ffn.masses_for(ff)
    pos = x[:3].astype(np.float64) * to_nm
    E = ffn.forces_nm(pos, ff)[2]
    pos = pos[np.argsort(-E)]                                    # descending energy up the ladder: every exchange is accepted
    T, ids = np.float32([300.0, 600.0, 1200.0]), np.arange(3, dtype=np.int64) + 7
    vel = ffn.draw_velocities(T, ids, m, 3, 0, numpy_normal)
    kw = dict(ff=ff, masses=m, dt=1e-6, friction=0.0, seed=3, to_nm=to_nm, normal=None)
    p1, v1, _, _, _ = ffn.langevin(pos, vel, T, ids, n_steps=1, **kw)
    out = rn.remd(pos, vel, T, ids, None, 3, 1, n_steps=1, step_offset=1, **kw)          # attempt 2: the pair (0, 1)
    assert out[5].tolist() == [1, 0, 2] and out[6].tolist() == [[1, 0, 2]] and out[7].tolist() == [[[1, 1], [0, 0]]]
    assert np.array_equal(out[0], p1[[1, 0, 2]])
    h = 0.5e-6 * ffn.forces_nm(p1, ff)[0] / m[None, :, None]     # half a kick: the velocity at the positions' time is v + h
    assert np.abs(h).max() > 0
    assert np.array_equal(out[1][0], (v1[1] + h[1]) * np.sqrt(300.0 / 600.0) - h[1])
    assert np.array_equal(out[1][1], (v1[0] + h[0]) * np.sqrt(600.0 / 300.0) - h[0]) and np.array_equal(out[1][2], v1[2])
    plain = rn.remd(pos, vel, T, ids, None, 3, 1, n_steps=1, step_offset=1, stored=True, **kw)      # the stored velocity rescaled as it is
    assert np.array_equal(plain[1][0], v1[1] * np.sqrt(300.0 / 600.0)) and np.array_equal(plain[0], out[0])
    same = rn.remd(pos, vel, T, ids, None, 3, 5, n_steps=3, stride=1, step_offset=1, **kw)      # g = 2, 3, 4: no attempt
    ref = ffn.langevin(pos, vel, T, ids, n_steps=3, stride=1, step_offset=1, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(same[:5], ref)) and same[6].shape == (0, 3) and not same[7].any()
    # chained calls run the same attempts as one call
    whole = rn.remd(pos, vel, T, ids, None, 3, 2, n_steps=5, stride=2, step_offset=3, **kw)
    a = rn.remd(pos, vel, T, ids, None, 3, 2, n_steps=2, stride=2, step_offset=3, **kw)
    b = rn.remd(a[0], a[1], T, ids, None, 3, 2, n_steps=3, stride=2, step_offset=5, walker=a[5], **kw)
    assert np.array_equal(b[0], whole[0]) and np.array_equal(b[1], whole[1]) and np.array_equal(b[5], whole[5])
    assert np.array_equal(np.concatenate([a[6], b[6]]), whole[6]) and np.array_equal(a[7] + b[7], whole[7]) and len(whole[6]) == 3


def test_the_velocity_is_rescaled_at_the_positions_time():
    """Why the exchange rescales v + (dt / 2) f / m and not the stored v.  A one-dimensional harmonic bond (k = 2.09e5 kJ / (mol nm^2),
    reduced mass 6, dt = 1 fs, friction 0.1 / ps: the GPU physics test's numbers) in the integrator's scheme, 4000 ladders of 300 /
    1000 K from equilibrium, an attempt every 14 steps, 8000 steps, frames every 20 after the first 2000.  The scheme stores the
    velocity half a kick behind the positions, so it is correlated with x; rescaling it as it is loses energy at every exchange, and
    at this friction the loss accumulates.  <x^2> k / (R T) at the cold rung: 1 with the rescale at the positions' time, well below
    1 with the stored velocity rescaled."""
    k, mu, dt, a = 2.09e5, 6.0, 1e-3, np.exp(-0.1 * 1e-3)
    T = np.array([300.0, 1000.0])
    beta, N = 1.0 / (fn.R_GAS * T), 4000
    amp, s01 = np.sqrt((1 - a * a) * fn.R_GAS * T / mu), np.sqrt(T[0] / T[1])

    def run(mode):
        rs = np.random.RandomState(0)
        x, v = rs.standard_normal((N, 2)) * np.sqrt(fn.R_GAS * T / k), rs.standard_normal((N, 2)) * np.sqrt(fn.R_GAS * T / mu)
        v = v - 0.5 * dt * (-k * x) / mu                          # the stored velocity of an equilibrium state
        acc, n = np.zeros(2), 0
        for s in range(1, 8001):
            v = v + dt * (-k * x) / mu
            x = x + 0.5 * dt * v
            v = a * v + amp * rs.standard_normal((N, 2))
            x = x + 0.5 * dt * v
            if s > 2000 and s % 20 == 0:
                acc, n = acc + (x * x).mean(axis=0), n + 1
            if mode and s % 14 == 0:
                E = 0.5 * k * x * x
                ok = np.log(rs.random_sample(N)) < (beta[0] - beta[1]) * (E[:, 0] - E[:, 1])
                h = 0.5 * dt * (-k * x) / mu if mode == "on_step" else np.zeros_like(x)
                x0, x1, v0, v1 = x[:, 0].copy(), x[:, 1].copy(), v[:, 0].copy(), v[:, 1].copy()
                x[:, 0], x[:, 1] = np.where(ok, x1, x0), np.where(ok, x0, x1)
                v[:, 0], v[:, 1] = np.where(ok, (v1 + h[:, 1]) * s01 - h[:, 1], v0), np.where(ok, (v0 + h[:, 0]) / s01 - h[:, 0], v1)
        return acc / n * k / (fn.R_GAS * T)

    on_step, stored = run("on_step"), run("stored")               # measured: [0.999, 0.995] and [0.852, 0.752]
    print(f"<x^2> k / (R T) at 300 / 1000 K: rescaled at the positions' time {on_step}, stored velocity rescaled {stored}")
    assert np.abs(on_step - 1).max() < 0.03 and stored[0] < 0.93


# ---- 3. the fixture of the GPU trajectory test ---------------------------------------------------------------------------------------
TRAJ = dict(dt=5e-4, friction=1.0, n_steps=16, stride=4, seed=11)
TRAJ_T = np.float32([300.0, 310.0, 320.0])
TRAJ_EVERY, TRAJ_K, TRAJ_LADDERS = 4, 3, 3


@functools.lru_cache(maxsize=None)
def trajectory_case(name, ft=np.float64):
    """(inputs, the restatement's run) of the GPU trajectory test: A4 / A9, three ladders of three rungs, 16 steps, an attempt every 4"""
    ff, x, to_nm = next((ff, x, to_nm) for n, ff, x, to_nm in fixtures() if n == name)
    m = ffn.masses_for(ff)
    B = TRAJ_K * TRAJ_LADDERS
    pos = x[:B].astype(np.float64) * to_nm
    T, ids, lids = np.tile(TRAJ_T, TRAJ_LADDERS), np.arange(B, dtype=np.int64) * 3 + 7, np.arange(TRAJ_LADDERS, dtype=np.int64) + 5
    out = rn.remd(pos, None, T, ids, lids, TRAJ_K, TRAJ_EVERY, ff, m, to_nm=to_nm, draw=True, ft=ft, **TRAJ)
    return (ff, m, pos, T, ids, lids, to_nm), out


@pytest.mark.parametrize("name", ["A4", "A9"])
def test_no_decision_of_the_trajectory_fixture_is_marginal(name):
    """what makes the GPU comparison of a whole trajectory valid: in the restatement alone every decision of the run has
    |logu - delta| > 1e-6, and the run has at least one acceptance and one rejection"""
    _, out = trajectory_case(name)
    counts, margins = out[7], out[8]
    print(f"{name}: {counts[..., 0].sum()} decisions, {counts[..., 1].sum()} accepted, smallest |logu - delta| = {margins.min():.3e}")
    assert len(margins) == counts[..., 0].sum() == TRAJ_LADDERS * 4 and margins.min() > 1e-6
    assert 0 < counts[..., 1].sum() < counts[..., 0].sum()


# ---- 4. round trips -----------------------------------------------------------------------------------------------------------------
def test_round_trips():
    ti = pkg()
    rt = ti.md.round_trips
    ident = [0, 1, 2]
    assert rt(np.array([ident] * 4)).tolist() == [0]
    # configuration 0 climbs to the top and comes back: one trip; configuration 2 only went down and up again: none
    hist = np.array([[1, 0, 2], [1, 2, 0], [1, 0, 2], [0, 1, 2]])
    assert rt(hist).tolist() == [1]
    twice = np.concatenate([hist, hist])
    assert rt(twice).tolist() == [2]
    two = np.stack([twice, np.array([ident] * 8)], axis=1)      # [n, 2 ladders, K]
    assert rt(two).tolist() == [2, 0] and rt(two).dtype == np.int64
    # K = 2, an exchange at every attempt.  Configuration 0: bottom, top (t = 0), bottom (1), top (2), bottom (3): two trips;
    # configuration 1: first at the bottom at t = 0, top (1), bottom (2): one
    k2 = np.array([[1, 0], [0, 1], [1, 0], [0, 1]])
    assert rt(k2).tolist() == [3]
    assert rt(np.zeros((0, 3, 4), np.int32)).tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="walkers"):
        rt(np.zeros(4))


# ---- 5. the driver ------------------------------------------------------------------------------------------------------------------
class StubRemdEngine(StubEngine):
    """StubEngine plus what md.ReplicaExchangeSampler asks for; the frames carry (replica id, frame step, T) as there"""

    def remd(self, pos, vel, T, n_rungs, exchange_every, dt, friction, n_steps, stride=0, step_offset=0, seed=0, ids=None, ladder_ids=None,
             walker=None, **kw):
        out = self.langevin(pos, vel, T, dt, friction, n_steps, stride=stride, step_offset=step_offset, seed=seed, ids=ids, **kw)
        self.calls[-1].update(K=n_rungs, every=exchange_every, ladder_ids=np.array(ladder_ids), walker=np.array(walker))
        B = len(pos)
        n_att = (step_offset + n_steps) // exchange_every - step_offset // exchange_every
        cnt = np.zeros((B // n_rungs, n_rungs - 1, 2), np.int64)
        cnt[..., 0], cnt[:, 0, 1] = n_att, n_att
        w = np.array(walker)
        hist = []
        for _ in range(n_att):                                  # every attempt swaps rungs 0 and 1 of every ladder
            w = w.reshape(-1, n_rungs).copy()
            w[:, [0, 1]] = w[:, [1, 0]]
            hist.append(w.reshape(-1))
            w = hist[-1]
        return (*out, w.reshape(-1), np.array(hist, np.int32).reshape(n_att, B), cnt)


def test_generate_md_with_exchange_permutes_to_ladders_and_back(tmp_path):
    ti = pkg()
    cfg, x0 = md_config(tmp_path, temperatures=[1000, 300, 500], exchange_every=2)
    eng = StubRemdEngine()
    paths = ti.drivers.generate_md(cfg, eng)
    draw, equil, run = eng.calls
    # ladder r = the rows (T_k, replica r) in ascending temperature; every row keeps the id k * n_replicas + r of the other path
    assert run["T"].tolist() == [300.0, 500.0, 1000.0] * 5 and run["K"] == 3 and run["every"] == 2 and run["ladder_ids"].tolist() == list(range(5))
    assert run["ids"].tolist() == [k * 5 + r for r in range(5) for k in (1, 2, 0)]
    np.testing.assert_array_equal(draw["pos"], (x0[np.arange(15) % 2] * 0.1)[run["ids"]])
    assert (equil["n_steps"], equil["step_offset"], run["n_steps"], run["stride"], run["step_offset"]) == (7, 0, 6, 2, 7)
    assert equil["walker"].tolist() == [0, 1, 2] * 5 and run["walker"].tolist() == [1, 0, 2] * 5     # 3 attempts in 7 steps: carried over
    first = 0
    for split, n in (("train", 3), ("val", 1), ("test", 1)):
        a = np.load(paths[split])
        assert a.shape == (8, n * 3, 5, 3) and np.isnan(a[[1, 3, 4, 5, 6]]).all()
        for row, k, temp in ((0, 1, 300.0), (2, 2, 500.0), (7, 0, 1000.0)):                            # today's layout: id = k * 5 + replica
            np.testing.assert_array_equal(a[row, :, 0, 0], np.repeat(k * 5 + first + np.arange(n), 3))
            assert (a[row, :, 0, 2] == temp).all()
        first += n
    with np.load(os.path.join(cfg.traj_path, "md_log.npz")) as z:
        assert int(z["exchange_every"]) == 2 and z["accept_counts"].shape == (5, 2, 2) and z["round_trips"].shape == (5,)
        assert z["accept_counts"][..., 0].tolist() == [[6, 6]] * 5 and z["accept_counts"][:, 0, 1].tolist() == [6] * 5      # 3 + 3 attempts
        np.testing.assert_array_equal(z["epot"][1, :, 0], 5 + np.arange(5))                              # epot in today's order too


def test_generate_md_without_the_key_is_todays_path(tmp_path):
    ti = pkg()
    logs = []
    for sub, over in (("a", {}), ("b", dict(exchange_every=0))):
        os.makedirs(tmp_path / sub)
        cfg, _ = md_config(tmp_path / sub, **over)
        eng = StubRemdEngine()
        paths = ti.drivers.generate_md(cfg, eng)
        assert all("K" not in c for c in eng.calls) and len(eng.calls) == 3
        with np.load(os.path.join(cfg.traj_path, "md_log.npz")) as z:
            assert not {"exchange_every", "accept_counts", "round_trips"} & set(z.files)
            logs.append({k: z[k] for k in z.files})
        logs.append({s: np.load(p) for s, p in paths.items()})
    for a, b in ((logs[0], logs[2]), (logs[1], logs[3])):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a)


@pytest.mark.parametrize("over,named", [(dict(exchange_every=-1), "exchange_every"), (dict(exchange_every=2.5), "exchange_every"),
                                        (dict(exchange_every=True), "exchange_every"), (dict(exchange_every=3, temperatures=[300]), "two")])
def test_generate_md_checks_the_exchange_key_before_it_runs(tmp_path, over, named):
    ti = pkg()
    cfg, _ = md_config(tmp_path, **over)
    eng = StubRemdEngine()
    with pytest.raises(ValueError, match=named):
        ti.drivers.generate_md(cfg, eng)
    assert not eng.calls and not os.path.exists(cfg.traj_path)
