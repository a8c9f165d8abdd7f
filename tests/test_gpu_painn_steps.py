"""Whole epochs of the molecule trainer on the GPU (ti_painn_train_steps, ti_painn_train_best, ti_painn_train_noise): a many-step call
against the loop of single steps bit for bit, the skip inside a sequence, the best-weights rule, the forward-only pass, the latent base
samples against the numpy restatement and the scipy fixture, and the Python path down to the drivers."""
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import painn_noise_numpy as pn
import painn_train_cases as pc
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu

F, B, N0, N1, STEPS = 32, 5, 23, 31, 7
SEED, OFF, DRAW = 77, (1 << 32) + 9, 40            # ids above 2^32: the high counter word of the draws


def _pool(variant, kind, A, L, seed=0, center="batch", F=F, B=B, N0=N0, N1=N1):
    """A model and two resident sets of 23 and 31 molecules with their temperatures, and [7, 5] indices that cross both sets
    unevenly: a row that holds one molecule twice, and molecules that come back in a later step (other F, B and set sizes on request)"""
    c = pc.make_case(variant, F, L, A, N1, tpl="sparse", kind=kind, gamma="sin2", center=center, seed=seed)
    rs = np.random.RandomState(50 + seed)
    c["set0"], c["set1"] = np.ascontiguousarray(c["x0"][:N0]), np.ascontiguousarray(c["x1"])
    c["temp0"] = (300.0 + 100.0 * (np.arange(N0) % 8)).astype(np.float32)
    c["temp1"] = (300.0 + 100.0 * (np.arange(N1) % 6)).astype(np.float32)
    i0 = np.stack([rs.permutation(N0)[:B] for _ in range(STEPS)]).astype(np.int64)
    i1 = np.stack([rs.permutation(N1 - 1)[:B] for _ in range(STEPS)]).astype(np.int64)      # the last molecule is kept for the NaN test
    i0[1, 3] = i0[1, 0]; i1[2, 4] = i1[2, 1]                                                # a molecule twice in one minibatch
    i0[5] = i0[0][::-1]; i1[6, :3] = i1[0, :3]                                              # molecules reused by a later step
    c["idx0"], c["idx1"] = i0, i1
    c["ncond"] = {0: 2, 1: 1, 2: 0}[variant]
    c["batch"] = B
    c["kw"] = dict(kind=kind, gamma="sin2", a=1.0, center=center, t_distr="beta_half", seed=SEED, traj_offset=OFF)
    return c


def _temps(c):
    return (c["temp0"] if c["ncond"] == 2 else None), (c["temp1"] if c["ncond"] >= 1 else None)


def _cond(c, r0, r1):
    A = c["A"]
    if c["ncond"] == 0:
        return None
    cols = [c["temp0"][r0], c["temp1"][r1]] if c["ncond"] == 2 else [c["temp1"][r1]]
    return np.ascontiguousarray(np.stack([np.repeat(v[:, None], A, axis=1) for v in cols], axis=-1).astype(np.float32))


def _loop(tr, c, idx0, idx1, x1=None, draw=DRAW, states=None):
    """ti_painn_train_step on the host-gathered rows of every step -> (losses, skipped)"""
    x1 = c["set1"] if x1 is None else x1
    losses, skipped = [], 0
    for k in range(idx0.shape[0]):
        if states is not None:
            states.append(tr.state()["w"])
        m, s = tr.step(np.ascontiguousarray(c["set0"][idx0[k]]), np.ascontiguousarray(x1[idx1[k]]), _cond(c, idx0[k], idx1[k]), draw=draw + k, **c["kw"])
        losses.append(m); skipped += s
    return np.asarray(losses), skipped


def _same_state(a, b):
    sa, sb = a.state(), b.state()
    return all(np.array_equal(sa[q], sb[q]) for q in "wmv") and sa["n_applied"] == sb["n_applied"] and sa["n_skipped"] == sb["n_skipped"]


CASES = [(0, "standard", 7, 2), (0, "one_sided", 3, 1), (1, "standard", 3, 1), (1, "one_sided", 7, 2), (2, "standard", 7, 1), (2, "one_sided", 3, 2)]
# the trainer's edges (tests/painn_train_cases.py EDGE_MATRIX) through this entry point: F = 256, and a minibatch of 683 molecules of
# three atoms from sets of 690 and 700, whose 2049 node rows and 6147 vector rows lie one row and one triple over a slice
EDGE_CASES = [((0, "standard", 3, 1), dict(F=256), "F256"), ((1, "one_sided", 3, 1), dict(B=683, N0=690, N1=700), "B683")]


# ------------------------------------------------------------------------------------------------ steps equal the loop
@pytest.mark.parametrize("variant,kind,A,L,shape", [case + ({},) for case in CASES] + [case + (shape,) for case, shape, _ in EDGE_CASES],
                         ids=[f"v{v}-{k}-A{a}-L{l}" for v, k, a, l in CASES] + [f"v{v}-{k}-A{a}-L{l}-{tag}" for (v, k, a, l), _, tag in EDGE_CASES])
def test_steps_equal_the_loop_of_single_steps(variant, kind, A, L, shape):
    """One call on host sets, one on device sets and indices, and seven ti_painn_train_step calls on the host-gathered rows: the same
    master weights, moments, counters and losses, bit for bit.  Then n_steps = 1 without indices against a step on rows 0..B-1."""
    c = _pool(variant, kind, A, L, seed=variant + (0 if kind == "standard" else 3), center="molecule" if variant == 1 else "batch", **shape)
    B = c["batch"]
    if "B" in shape:
        S = pkg()._lib.PAINN_TRAIN_SLICE
        assert kind == "one_sided" and B * A == S + 1 and 3 * B * A == 3 * S + 3          # node and vector rows one over a slice
    t0, t1 = _temps(c)
    host, loop, dev = (pc.make_trainer(c, lr=1e-3) for _ in range(3))
    lh, sh = host.steps(c["set0"], c["set1"], t0, t1, c["idx0"], c["idx1"], draw=DRAW, **c["kw"])
    ll, sl = _loop(loop, c, c["idx0"], c["idx1"])
    cu = lambda v: None if v is None else torch.from_numpy(v).cuda()
    ld, sd = dev.steps(cu(c["set0"]), cu(c["set1"]), cu(t0), cu(t1), cu(c["idx0"]), cu(c["idx1"]), draw=DRAW, **c["kw"])
    print(f"losses {lh}")
    assert np.isfinite(lh).all() and sh == sl == sd == 0
    assert np.array_equal(lh, ll) and np.array_equal(lh, ld)
    assert _same_state(host, loop) and _same_state(host, dev) and host.state()["n_applied"] == STEPS
    assert not np.array_equal(host.state()["w"], c["flat"])
    l1, s1 = host.steps(c["set0"], c["set1"], t0, t1, batch=B, draw=DRAW + 20, **c["kw"])
    r = np.arange(B)
    m1, _ = loop.step(np.ascontiguousarray(c["set0"][:B]), np.ascontiguousarray(c["set1"][:B]), _cond(c, r, r), draw=DRAW + 20, **c["kw"])
    assert l1.shape == (1,) and l1[0] == m1 and s1 == 0 and _same_state(host, loop)


# ------------------------------------------------------------------------------------------------ the skip, the best weights
def test_a_skip_inside_a_sequence_and_the_best_weights():
    """Pool molecule 30 is NaN and used by step 3 only: that loss is NaN, one step is skipped, six are applied, and the rest equals the
    loop that makes the same skip (the bias table is indexed by the device counter).  ti_painn_train_best: the first strict minimum of
    the returned losses, and the master weights as get_state gave them BEFORE that step in the replayed loop."""
    ti = pkg()
    c = _pool(0, "standard", 7, 1, seed=6)
    t0, t1 = _temps(c)
    x1 = c["set1"].copy()
    x1[N1 - 1, 2, 1] = np.nan
    idx1 = c["idx1"].copy()
    idx1[3, 2] = N1 - 1
    a, b = pc.make_trainer(c, lr=1e-3), pc.make_trainer(c, lr=1e-3)
    with pytest.raises(ti._lib.TiError) as ei:
        a.best()
    assert ei.value.code == ti._lib.TI_E_ARG
    la, sa = a.steps(c["set0"], x1, t0, t1, c["idx0"], idx1, draw=DRAW, track_best=True, **c["kw"])
    before = []
    lb, sb = _loop(b, c, c["idx0"], idx1, x1=x1, states=before)
    print(f"losses {la}")
    assert np.isnan(la[3]) and np.isfinite(np.delete(la, 3)).all() and sa == sb == 1
    assert np.array_equal(np.delete(la, 3), np.delete(lb, 3)) and np.isnan(lb[3])
    assert _same_state(a, b) and a.state()["n_applied"] == 6 and a.state()["n_skipped"] == 1
    best = a.best()
    want = int(np.nanargmin(la))                                # the first index of the smallest returned loss
    assert best["step"] == want != 3 and best["loss"] == la[want] and np.array_equal(best["w"], before[want])
    assert not np.array_equal(best["w"], a.state()["w"])
    # more steps without tracking leave it; a reset forgets it; the next tracking call counts from 0 again
    a.steps(c["set0"], c["set1"], t0, t1, c["idx0"][:2], c["idx1"][:2], draw=DRAW + 7, **c["kw"])
    again = a.best(reset=True)
    assert again["step"] == want and np.array_equal(again["w"], best["w"])
    with pytest.raises(ti._lib.TiError) as ei:
        a.best()
    assert ei.value.code == ti._lib.TI_E_ARG
    w0 = a.state()["w"]
    l2, _ = a.steps(c["set0"], c["set1"], t0, t1, c["idx0"][:3], c["idx1"][:3], draw=DRAW + 9, track_best=True, **c["kw"])
    l3, _ = a.steps(c["set0"], c["set1"], t0, t1, c["idx0"][3:5], c["idx1"][3:5], draw=DRAW + 12, track_best=True, **c["kw"])
    both = np.concatenate([l2, l3])
    nb = a.best()
    assert nb["step"] == int(np.argmin(both)) and nb["loss"] == both.min()          # the count runs over the calls since the reset
    if nb["step"] == 0:
        assert np.array_equal(nb["w"], w0)


# ------------------------------------------------------------------------------------------------ forward only
@pytest.mark.parametrize("variant,kind", [(0, "standard"), (1, "one_sided")])
def test_forward_only_steps_are_the_grad_means_and_change_nothing(variant, kind):
    c = _pool(variant, kind, 7, 2, seed=8)
    t0, t1 = _temps(c)
    tr = pc.make_trainer(c, lr=1e-3)
    tr.steps(c["set0"], c["set1"], t0, t1, c["idx0"][:2], c["idx1"][:2], draw=3, **c["kw"])          # off the starting point
    before = tr.state()
    losses, skipped = tr.steps(c["set0"], c["set1"], t0, t1, c["idx0"], c["idx1"], draw=DRAW, update=False, **c["kw"])
    after = tr.state()
    assert skipped == 0 and all(np.array_equal(before[q], after[q]) for q in "wmv")
    assert before["n_applied"] == after["n_applied"] == 2 and before["n_skipped"] == after["n_skipped"]
    for k in range(STEPS):
        r0, r1 = c["idx0"][k], c["idx1"][k]
        g = tr.grad(np.ascontiguousarray(c["set0"][r0]), np.ascontiguousarray(c["set1"][r1]), _cond(c, r0, r1), draw=DRAW + k, **c["kw"])
        assert losses[k] == g["mean"], k
    assert np.array_equal(tr.state()["w"], before["w"])


# ------------------------------------------------------------------------------------------------ the base samples
def _noise_trainer(A, variant=1):
    return pc.make_trainer(pc.make_case(variant, F, 1, A, 1, tpl="sparse", kind="one_sided", seed=2))


def test_drawn_noise_is_the_restatement_exactly():
    """out_x0 = fp32(x - mean) with the fp64 sum in atom order: exact against tests/painn_noise_numpy.py, which draws with oracle.normal"""
    A, n = 7, 16
    tr = _noise_trainer(A)
    got = tr.noise(B=n, seed=SEED, traj_offset=OFF, draw=DRAW)
    want, _, xc = pn.noise(SEED, OFF, DRAW, None, False, A=A, B=n)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.abs(xc.sum(axis=1)).max() < 1e-14
    x1 = torch.zeros((n, A, 3), dtype=torch.float32, device="cuda")
    assert np.array_equal(tr.noise(x1, seed=SEED, traj_offset=OFF, draw=DRAW).cpu().numpy(), want)      # device memory, x1 not read


@pytest.mark.parametrize("g", ["a3", "a9"])
def test_aligned_noise_against_the_scipy_fixture(g):
    """|out_x0 - fp32(fixture)| <= 2^-23 max|coordinate of the molecule|: both sides round an fp64 result once, and with the fixture's
    eigenvalue gap the fp64 results agree far below an fp32 ulp.  out_rot within 1e-10 of scipy's R, det = 1 within 1e-12."""
    z = load_golden("painn_noise_align")
    x1, want, R = z[f"x1_{g}"], z[f"aligned_{g}"], z[f"rot_{g}"]
    n, A = x1.shape[:2]
    seed, off, draw = int(z["seed"]), int(z[f"traj_offset_{g}"]), int(z["draw"])
    tr = _noise_trainer(A)
    got, rot = tr.noise(x1, aligned=True, seed=seed, traj_offset=off, draw=draw, return_rot=True)
    drawn = tr.noise(B=n, seed=seed, traj_offset=off, draw=draw)
    assert np.array_equal(drawn, z[f"x0_{g}"].astype(np.float32))
    bar = 2.0 ** -23 * np.abs(want).max(axis=(1, 2), keepdims=True)
    err = np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64))
    print(f"{g}: max err / bar {np.max(err / bar):.3f}; max |R - scipy| {np.abs(rot - R).max():.3e}; max |det - 1| {np.abs(np.linalg.det(rot) - 1).max():.3e}")
    assert (err <= bar).all()
    assert np.abs(rot - R).max() <= 1e-10 and np.abs(np.linalg.det(rot) - 1.0).max() <= 1e-12
    if g == "a9":
        assert np.abs(rot[0] - np.eye(3)).max() <= 1e-6                                    # x1 = x0 up to its float32 rounding
        K = x1[1].astype(np.float64).T @ z["x0_a9"][1]
        U, _, Vt = np.linalg.svd(K)
        assert np.linalg.det(U @ Vt) < 0.0 < np.linalg.det(rot[1])                         # the mirror molecule: the correction decided
    # a molecule's bits depend on its global index and its x1 alone: alone, and at another position with traj_offset shifted to match
    j = n - 2
    one, r1 = tr.noise(x1[j:j + 1], aligned=True, seed=seed, traj_offset=off + j, draw=draw, return_rot=True)
    part, rp = tr.noise(x1[j - 2:], aligned=True, seed=seed, traj_offset=off + j - 2, draw=draw, return_rot=True)
    assert np.array_equal(one[0], got[j]) and np.array_equal(r1[0], rot[j])
    assert np.array_equal(part[2], got[j]) and np.array_equal(rp[2], rot[j])
    dev, rd = tr.noise(torch.from_numpy(x1).cuda(), aligned=True, seed=seed, traj_offset=off, draw=draw, return_rot=True)
    assert np.array_equal(dev.cpu().numpy(), got) and np.array_equal(rd.cpu().numpy(), rot)


def test_noise_inside_a_batch_of_16():
    """B = 1 against the same molecule inside B = 16"""
    A = 9
    tr = _noise_trainer(A)
    x1 = np.random.RandomState(3).standard_normal((16, A, 3)).astype(np.float32)
    full = tr.noise(x1, aligned=True, seed=5, traj_offset=1000, draw=2)
    for j in (0, 7, 15):
        assert np.array_equal(tr.noise(x1[j:j + 1], aligned=True, seed=5, traj_offset=1000 + j, draw=2)[0], full[j])


@pytest.mark.parametrize("noise", ["aligned", "drawn"])
def test_latent_steps_draw_their_noise_like_the_loop(noise):
    """ti_painn_train_steps(noise) against ti_painn_train_noise with draw + k followed by ti_painn_train_step with that x0, bit for bit"""
    c = _pool(1, "one_sided", 7, 2, seed=12)
    a, b = pc.make_trainer(c, lr=1e-3), pc.make_trainer(c, lr=1e-3)
    la, sa = a.steps(None, c["set1"], None, c["temp1"], None, c["idx1"], draw=DRAW, noise=noise, **c["kw"])
    lb = []
    for k in range(STEPS):
        r1 = c["idx1"][k]
        x1 = np.ascontiguousarray(c["set1"][r1])
        x0 = b.noise(x1, aligned=noise == "aligned", seed=SEED, traj_offset=OFF, draw=DRAW + k)
        lb.append(b.step(x0, x1, _cond(c, r1, r1), draw=DRAW + k, **c["kw"])[0])
    assert sa == 0 and np.isfinite(la).all() and np.array_equal(la, np.asarray(lb)) and _same_state(a, b)


def test_refusals_that_need_a_trainer():
    ti = pkg()
    E = ti._lib
    c = _pool(0, "one_sided", 3, 1)
    amb = pc.make_trainer(c)
    with pytest.raises(E.TiError) as ei:                        # the ambient variant's set 0 is data
        amb.steps(None, c["set1"], c["temp1"], c["temp1"], None, c["idx1"], noise="drawn", **c["kw"])
    assert ei.value.code == E.TI_E_UNSUPPORTED
    with pytest.raises(E.TiError) as ei:                        # a missing temperature array
        amb.steps(c["set0"], c["set1"], None, c["temp1"], c["idx0"], c["idx1"], **c["kw"])
    assert ei.value.code == E.TI_E_ARG and "temperature" in str(ei.value)
    bad = torch.from_numpy(c["idx0"]).cuda()
    bad[4, 1] = N0                                              # a device index outside its set: refused before anything is enqueued
    cu = lambda v: torch.from_numpy(v).cuda()
    with pytest.raises(E.TiError) as ei:
        amb.steps(cu(c["set0"]), cu(c["set1"]), cu(c["temp0"]), cu(c["temp1"]), bad, cu(c["idx1"]), **c["kw"])
    assert ei.value.code == E.TI_E_ARG and "idx0[21]" in str(ei.value) and amb.state()["n_applied"] == 0
    two = pc.make_trainer(pc.make_case(2, F, 1, 2, 1, tpl="full", kind="one_sided"))
    x1 = np.zeros((4, 2, 3), np.float32)
    with pytest.raises(E.TiError) as ei:
        two.noise(x1, aligned=True)
    assert ei.value.code == E.TI_E_UNSUPPORTED
    with pytest.raises(E.TiError) as ei:
        two.steps(None, x1, None, None, noise="aligned", batch=4, kind="one_sided")
    assert ei.value.code == E.TI_E_UNSUPPORTED
    assert two.noise(B=4).shape == (4, 2, 3)                    # drawn noise has no such limit


# ------------------------------------------------------------------------------------------------ the Python path, once
def _template(m, A, n=2):
    ti = pkg()
    return SimpleNamespace(x=np.zeros((n * A, 3), np.float32), T=np.full(n * A, 300.0, np.float32), atoms=np.tile(m["atom_ids"], n).astype(np.int64),
                           edge_index=ti.synthetic.batch_edge_index(m["src"], m["dst"], A, n), edge_type=np.tile(m["etype"], n).astype(np.int64),
                           batch=np.repeat(np.arange(n), A))


def test_the_python_path_fit_evaluate_best_and_the_driver(tmp_path):
    ti = pkg()
    amb = import_module("thermodynamic-interpolation_amd.thermo.ambient")
    A, L = 3, 1
    c = _pool(0, "standard", A, L, seed=4)
    m = c["model"]
    tpl = _template(m, A)
    b = amb.cPaiNN(n_features=F, score_layers=L)
    b.load_state_dict(ti.weights.unflatten(c["flat"], c["spec"]))
    loss_fn = amb.losses.StandardVelocityLoss(amb.interpolants.LinearInterpolant(a=1.0, gamma="sin2"))
    tr = amb.Trainer(b, loss_fn, lr=1e-3)
    sets = (c["set0"], c["temp0"], c["set1"], c["temp1"])
    l1, s1 = tr.fit(*sets, B, 4, [3, 0], draw=0, noise_seed=3, template_batch=tpl)
    l2, s2 = tr.fit(*sets, B, 4, [3, 1], draw=4, noise_seed=3)
    ev = tr.evaluate(*sets, B, 4, [3, 1], draw=8, noise_seed=3)
    assert l1.shape == l2.shape == ev.shape == (4,) and s1 == s2 == 0 and np.isfinite(np.concatenate([l1, l2, ev])).all()
    assert tr.engine.state()["n_applied"] == 8
    sd, loss, step = tr.best_state_dict()
    both = np.concatenate([l1, l2])
    assert step == int(np.argmin(both)) and loss == both.min() and set(sd) == {k for k, _ in c["spec"]}
    assert tr.sync() is b and np.array_equal(ti.weights.flatten_state_dict(b.state_dict(), c["spec"]), tr.engine.weights().astype(np.float32))

    def config(n_epochs, name):
        return SimpleNamespace(n_features=F, score_layers=L, batch_size=B, n_epochs=n_epochs, learning_rate=1e-3, weight_decay=0.0, a=1.0,
                               gamma="sin2", t_distr="uniform", seed=5, align=False, model_save_path=str(tmp_path), model_save_name=name)
    set0, set1 = (c["set0"][:17], c["temp0"][:17]), (c["set1"][:19], c["temp1"][:19])          # 3 steps an epoch
    log = ti.drivers.train_ambient(config(2, "run"), set0, set1, tpl)
    out = os.path.join(str(tmp_path), "run")
    assert set(log) == {"train_loss", "last_train_loss", "best_loss", "lr", "skipped"} and all(v.shape == (2,) for v in log.values())
    with np.load(os.path.join(out, "log.npz")) as f:
        assert set(f.files) == set(log) and all(np.array_equal(f[k], log[k]) for k in log)
    assert (log["best_loss"] <= log["train_loss"]).all() and (log["skipped"] == 0).all()
    for name in ("run_0_weights.npz", "run_best0_weights.npz", "run_1_weights.npz", "run_best1_weights.npz"):
        fresh = amb.cPaiNN(n_features=F, score_layers=L)
        fresh.load_state_dict(ti.drivers._load_state_dict(os.path.join(out, name)))
    assert not np.array_equal(np.load(os.path.join(out, "run_1_weights.npz"))["net.8.layers.0.phi.mlp.0.weight"],
                              np.load(os.path.join(out, "run_best1_weights.npz"))["net.8.layers.0.phi.mlp.0.weight"])
    resumed = ti.drivers.train_ambient(config(3, "run"), set0, set1, tpl, resume=True)
    whole = ti.drivers.train_ambient(config(3, "whole"), set0, set1, tpl)
    assert all(np.array_equal(resumed[k], whole[k]) for k in whole)
    with np.load(os.path.join(out, "run_2_weights.npz")) as p, np.load(os.path.join(str(tmp_path), "whole", "whole_2_weights.npz")) as q:
        assert set(p.files) == set(q.files) and all(np.array_equal(p[k], q[k]) for k in p.files)
