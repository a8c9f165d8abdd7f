"""The molecule trainer on the GPU (ti_painn_train_*): gradients against the reference fixtures and against the torch restatement
over a shape matrix, bits, composition with the optimiser, the Python path, and the refusals that need a device."""
import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adw_train_numpy as an
import painn_train_cases as pc
from conftest import pkg
from test_gpu_vloss import _ref_bound

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(key, c):
    """(rows, mean, g64, g32) of the restatement, computed once per case and shared"""
    if key not in _REF:
        rows, mean, g64 = pc.reference(c)
        _, _, g32 = pc.reference(c, torch.float32)
        _REF[key] = (rows, mean, g64, g32)
    return _REF[key]


def _drift_engine(c):
    ti = pkg()
    m = c["model"]
    kw = dict(temp_length=m["temp_length"]) if "temp_length" in m else {}
    return ti.engine.PainnEngine(m["variant"], m["F"], m["L"], c["A"], m["src"], m["dst"], m["etype"], m["atom_ids"], c["flat"].astype(np.float32), **kw)


def _check_loss(c, r, rows64, mean64):
    """Loss rows and mean within the bound of tests/test_gpu_vloss.py, against fp64 and against ti_painn_vloss on an f32 drift handle
    of the same weights (whose drift, within 1e-5 of the truth like the trainer's, is what the bound is stated in)."""
    kw = pc.call_kw(c)
    v = _drift_engine(c).velocity_loss(c["x0"], c["x1"], c["cond"], returns=("b",), **kw)
    s = dict(kind=kw["kind"], gamma=kw["gamma"], a=kw["a"])
    cc = dict(t=c["t"], z=c["z"], bt_plus=v["b"][0], bt_minus=v["b"][-1])
    bound = _ref_bound(s, dict(x0=c["x0"], x1=c["x1"]), cc)
    rows = c["B"] * c["A"]
    for what, ref_rows, ref_mean in (("fp64", rows64, mean64), ("ti_painn_vloss", v["loss"], v["mean"])):
        print(f"   loss against {what}: max |dl| / bound {np.max(np.abs(r['loss'] - ref_rows) / bound):.3e}")
        assert (np.abs(r["loss"] - ref_rows) <= bound).all(), what
        assert abs(r["mean"] - ref_mean) <= bound.sum() / rows, what
    assert r["mean"] == pytest.approx(r["loss"].sum() / rows, rel=1e-14)


def _check_grad(c, r, g64, bars):
    got = pc.split(r["grad"], c["spec"])
    worst, budget = ("", 0.0, 1.0), 0.0
    for k, ref in g64.items():
        nr = np.linalg.norm(ref)
        if nr == 0.0:
            assert not np.any(got[k]), k
            continue
        e = float(np.linalg.norm(got[k] - ref) / nr)
        if e / bars[k] > worst[1] / worst[2]:
            worst = (k, e, bars[k])
        budget += (bars[k] * nr) ** 2
    print(f"   worst tensor {worst[0]}: {worst[1]:.3e} against a bar of {worst[2]:.3e}")
    for k, ref in g64.items():
        nr = np.linalg.norm(ref)
        if nr > 0.0:
            assert np.linalg.norm(got[k] - ref) / nr <= bars[k], (k, float(np.linalg.norm(got[k] - ref) / nr), bars[k])
    assert pc.zero_violations(got, g64) == []
    gn = np.sqrt(sum(float((v * v).sum()) for v in g64.values()))
    assert abs(r["gnorm"] - gn) <= np.sqrt(budget)            # the bar the tensors imply
    assert r["gnorm"] == pytest.approx(np.linalg.norm(r["grad"]), rel=1e-13)


# ------------------------------------------------------------------------------------------------ gradients against the fixtures
@pytest.mark.parametrize("name,case", pc.FIXTURE_CASES)
def test_gradients_against_the_reference(name, case):
    """Per tensor, rel-L2 against the reference's fp64 gradient <= max(1e-5, 3 x the reference's own float32 distance)."""
    c = pc.fixture_case(name, case)
    r = pc.make_trainer(c).grad(c["x0"], c["x1"], c["cond"], **pc.call_kw(c))
    print(f"{name} {case}: mean {r['mean']:.9f} (reference {float(c['mean64']):.9f})")
    assert all(d >= 0.0 for d in c["d32"].values())
    _check_grad(c, r, c["g64"], {k: max(1e-5, 3.0 * d) for k, d in c["d32"].items()})
    _check_loss(c, r, c["rows64"], float(c["mean64"]))


# ------------------------------------------------------------------------------------------------ a shape matrix against the restatement
def _check_cell(cell):
    """One cell of a shape matrix against the restatement: every tensor under its bar, the zero pattern, gnorm, the loss -> the case"""
    c = pc.matrix_case(cell)
    rows, mean, g64, g32 = _reference(cell, c)
    r = pc.make_trainer(c).grad(c["x0"], c["x1"], c["cond"], **pc.call_kw(c))
    print(f"{cell}: mean {r['mean']:.9f} (restatement {mean:.9f})")
    bars = {k: bar for k, _, bar in pc.tensor_errors(g32, g64, g32) if bar > 0.0}
    _check_grad(c, r, g64, bars)
    _check_loss(c, r, rows, mean)
    return c


@pytest.mark.parametrize("cell", pc.MATRIX, ids=pc.MATRIX_IDS)
def test_gradient_matrix(cell):
    c = _check_cell(cell)
    if cell[4] == 37 and cell[5] == "full":
        ti = pkg()
        n_rows = 2 * c["B"] * c["model"]["src"].size
        assert n_rows > 2 * ti._lib.PAINN_TRAIN_SLICE and n_rows % ti._lib.PAINN_TRAIN_SLICE      # three slices, the last one ragged


def _slice_premise(which, c):
    """The row counts the two slice cells are there for, stated against the library's constant: should the slice change, the cell
    says that its premise is gone."""
    S = pkg()._lib.PAINN_TRAIN_SLICE
    nodes, vectors, edges = pc.row_counts(c)
    if which == pc.EDGE_EXACT:                                # every row count a whole number of slices, none of them a single one but the nodes'
        assert nodes == S and vectors == 3 * S and edges % S == 0 and edges // S == 31
    elif which == pc.EDGE_ONE_OVER:                           # one node row and one vector triple over; the edge rows ragged in a second slice
        assert nodes == S + 1 and vectors == 3 * S + 3 and S < edges < 2 * S


@pytest.mark.parametrize("cell", pc.EDGE_MATRIX, ids=pc.EDGE_IDS)
def test_gradient_edge_matrix(cell):
    """The cells of pc.EDGE_MATRIX through the body of test_gradient_matrix, with the premises of the cells that are there for a
    row count: the slice cells, and R = 1 / 16 / 17 molecules against the 16 accumulators of the table and column sums."""
    c = _check_cell(cell)
    which = pc.EDGE_MATRIX.index(cell)
    _slice_premise(which, c)
    R = pc.halves(c["lk"]["kind"]) * c["B"]
    if which in (6, 7, 8):
        assert R == {6: 1, 7: 16, 8: 17}[which]
    if which == 6:
        assert R * c["A"] < 16                                # a single partial 16-row tile of the product kernel
    if which == 3:
        assert c["A"] == 32 and np.bincount(c["model"]["dst"]).min() == 31 and len(set(c["model"]["atom_ids"].tolist())) < c["A"]


# ------------------------------------------------------------------------------------------------ bits
def _bits_case():
    return pc.make_case(0, 32, 2, 7, 5, tpl="sparse", kind="standard", gamma="sin2", center="batch", seed=3)


def test_gradient_bits_do_not_depend_on_the_call():
    """The same call twice; host and device pointers; after a larger call; another row order gives other bits, the same gradient."""
    c = _bits_case()
    tr = pc.make_trainer(c)
    kw = pc.call_kw(c)
    a = tr.grad(c["x0"], c["x1"], c["cond"], **kw)
    b = tr.grad(c["x0"], c["x1"], c["cond"], **kw)
    same = lambda p, q: np.array_equal(p["grad"], q["grad"]) and np.array_equal(np.asarray(p["loss"]), np.asarray(q["loss"])) and p["mean"] == q["mean"]
    assert same(a, b)
    dev = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()
    kd = dict(kw, t=dev(kw["t"]), z=dev(kw["z"]))
    d = tr.grad(dev(c["x0"]), dev(c["x1"]), dev(c["cond"]), **kd)
    d["loss"] = d["loss"].cpu().numpy()
    assert same(a, d)
    big = pc.make_case(0, 32, 2, 7, 23, tpl="sparse", kind="standard", gamma="sin2", center="batch", seed=4)
    tr.grad(big["x0"], big["x1"], big["cond"], **pc.call_kw(big))
    assert same(a, tr.grad(c["x0"], c["x1"], c["cond"], **kw))
    perm = np.asarray([3, 0, 4, 1, 2])
    p = tr.grad(c["x0"][perm], c["x1"][perm], c["cond"][perm], **dict(kw, t=kw["t"][perm], z=kw["z"][perm]))
    assert np.allclose(p["loss"], a["loss"][perm], rtol=1e-4, atol=1e-6)
    assert not np.array_equal(p["grad"], a["grad"])
    ga, gp = pc.split(a["grad"], c["spec"]), pc.split(p["grad"], c["spec"])
    for k in ga:
        if np.any(ga[k]):
            assert np.linalg.norm(gp[k] - ga[k]) <= 1e-5 * np.linalg.norm(ga[k]), k


@pytest.mark.parametrize("which,more", [(pc.EDGE_EXACT, 1), (pc.EDGE_ONE_OVER, 17)], ids=["exact-multiple", "one-over"])
def test_gradient_bits_at_the_slice_edges(which, more):
    """The slices exist so that a gradient does not depend on the call: at a row count that is a whole number of slices and at one row
    over, the same call twice and again after a larger call on the same trainer give the same bits."""
    cell = pc.EDGE_MATRIX[which]
    c = pc.matrix_case(cell)
    _slice_premise(which, c)
    tr = pc.make_trainer(c)
    kw = pc.call_kw(c)
    a = tr.grad(c["x0"], c["x1"], c["cond"], **kw)
    b = tr.grad(c["x0"], c["x1"], c["cond"], **kw)
    same = lambda p, q: np.array_equal(p["grad"], q["grad"]) and np.array_equal(np.asarray(p["loss"]), np.asarray(q["loss"])) and p["mean"] == q["mean"]
    assert same(a, b) and np.isfinite(a["grad"]).all() and a["gnorm"] > 0.0
    big = pc.matrix_case(cell[:4] + (cell[4] + more,) + cell[5:11] + (cell[11] + 1,))
    g = tr.grad(big["x0"], big["x1"], big["cond"], **pc.call_kw(big))
    assert not np.array_equal(g["grad"], a["grad"])
    assert same(a, tr.grad(c["x0"], c["x1"], c["cond"], **kw))


def test_outputs_end_where_they_should():
    """Sentinels behind out_loss and out_grad stay as they are."""
    ti = pkg()
    c = _bits_case()
    tr = pc.make_trainer(c)
    kw = pc.call_kw(c)
    desc = tr._vloss_desc(kw["kind"], kw["gamma"], kw["a"], kw["center"], kw["t"], "uniform", 0, 0, 0, 0)
    B, n = c["B"], tr.n_weights
    loss, grad = np.full(B + 4, -7.25), np.full(n + 4, -7.25)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    mean, gnorm = C.c_double(0.0), C.c_double(0.0)
    ti._lib.check(ti._lib.lib().ti_painn_train_grad(tr.h, C.byref(desc), vp(c["x0"]), vp(c["x1"]), vp(c["cond"]), vp(kw["t"]), vp(kw["z"]), B,
                                                   vp(loss), C.byref(mean), dp(grad), C.byref(gnorm), ti._lib.MEM_HOST))
    assert (loss[B:] == -7.25).all() and (grad[n:] == -7.25).all()
    r = tr.grad(c["x0"], c["x1"], c["cond"], **kw)
    assert np.array_equal(loss[:B], r["loss"]) and np.array_equal(grad[:n], r["grad"]) and mean.value == r["mean"]


# ------------------------------------------------------------------------------------------------ composition
def test_step_is_grad_then_apply():
    c = _bits_case()
    kw = pc.call_kw(c)
    a, b = pc.make_trainer(c, lr=1e-3), pc.make_trainer(c, lr=1e-3)
    for k in range(3):
        r = a.grad(c["x0"], c["x1"], c["cond"], **kw)
        assert a.apply(r["grad"]) is False
        mean, skipped = b.step(c["x0"], c["x1"], c["cond"], **kw)
        assert mean == r["mean"] and skipped == 0
        sa, sb = a.state(), b.state()
        assert all(np.array_equal(sa[q], sb[q]) for q in "wmv") and sa["n_applied"] == sb["n_applied"] == k + 1
    assert not np.array_equal(sa["w"], c["flat"])


@pytest.mark.parametrize("max_norm,wd", [(1.0, 0.0), (1e3, 0.0), (0.0, 1e-5), (1.0, 1e-5)], ids=["clip-active", "clip-inactive", "clip-off-wd", "clip-wd"])
def test_apply_against_the_restated_optimiser(max_norm, wd):
    c = pc.fixture_case("painn_train_ambient", "brownian")
    lr = 1e-4
    tr = pc.make_trainer(c, lr=lr, max_grad_norm=max_norm, weight_decay=wd)
    opt = an.Adam(c["flat"], lr=lr, max_grad_norm=max_norm, weight_decay=wd)
    flat = np.concatenate([c["g64"][k].ravel() for k, _ in c["spec"]])
    assert np.linalg.norm(flat) > 1.0                         # the clip at 1 is active, the one at 1e3 is not
    for k in range(1, 4):
        assert tr.apply(flat * k) is False and not opt.step(flat * k)
        w = tr.weights()
        ratio = np.max(np.abs(w - opt.w) / an.adam_bound(opt.w, lr, k))
        print(f"step {k}: {ratio:.3f} of the bound")
        assert ratio <= 1.0
    st = tr.state()
    assert np.max(np.abs(st["m"] - opt.m)) <= 1e-14 * np.max(np.abs(opt.m)) and st["n_applied"] == 3


def test_an_inf_makes_a_skipped_step_that_leaves_everything():
    c = _bits_case()
    kw = pc.call_kw(c)
    tr = pc.make_trainer(c)
    tr.step(c["x0"], c["x1"], c["cond"], **kw)
    before = tr.state()
    x1 = c["x1"].copy()
    x1[2, 1, 0] = np.inf
    mean, skipped = tr.step(c["x0"], x1, c["cond"], **kw)
    after = tr.state()
    assert np.isnan(mean) and skipped == 1
    assert all(np.array_equal(before[q], after[q]) for q in "wmv") and after["n_applied"] == before["n_applied"] == 1
    assert after["n_skipped"] == before["n_skipped"] + 1
    bad = np.zeros(tr.n_weights)
    bad[5] = np.nan
    assert tr.apply(bad) is True and np.array_equal(tr.state()["w"], before["w"])
    mean, skipped = tr.step(c["x0"], c["x1"], c["cond"], **kw)             # and the following step goes on
    assert np.isfinite(mean) and skipped == 0 and tr.state()["n_applied"] == 2


def test_state_moves_into_a_new_trainer():
    c = _bits_case()
    kw = pc.call_kw(c)
    a = pc.make_trainer(c, lr=2e-3)
    for _ in range(2):
        a.step(c["x0"], c["x1"], c["cond"], **kw)
    b = pc.make_trainer(c, lr=2e-3)
    b.load_state(**a.state())
    ma, mb = a.step(c["x0"], c["x1"], c["cond"], **kw), b.step(c["x0"], c["x1"], c["cond"], **kw)
    sa, sb = a.state(), b.state()
    assert ma == mb and all(np.array_equal(sa[q], sb[q]) for q in "wmv") and sa["n_applied"] == sb["n_applied"] == 3
    a.set_lr(1e-4); b.set_lr(1e-4)
    a.step(c["x0"], c["x1"], c["cond"], **kw); b.step(c["x0"], c["x1"], c["cond"], **kw)
    assert np.array_equal(a.weights(), b.weights())


# ------------------------------------------------------------------------------------------------ the Python path
def test_ambient_trainer_lowers_the_loss_and_syncs():
    ti = pkg()
    amb = import_module("thermodynamic-interpolation_amd.thermo.ambient")
    F, L, A, B = 32, 2, 6, 8
    c = pc.make_case(0, F, L, A, B, kind="standard", gamma="brownian", a=0.9, center="batch", seed=9)
    m = c["model"]
    b = amb.cPaiNN(n_features=F, score_layers=L)
    b.load_state_dict(ti.weights.unflatten(c["flat"].astype(np.float32), c["spec"]))
    loss_fn = amb.losses.StandardVelocityLoss(amb.interpolants.LinearInterpolant(a=0.9, gamma="brownian"))
    ei = ti.synthetic.batch_edge_index(m["src"], m["dst"], A, B)
    mk = lambda x, T: SimpleNamespace(x=x.reshape(B * A, 3), T=T.reshape(B * A), atoms=np.tile(m["atom_ids"], B).astype(np.int64), edge_index=ei,
                                      edge_type=np.tile(m["etype"], B).astype(np.int64), batch=np.repeat(np.arange(B), A))
    batch0, batch1 = mk(c["x0"], c["cond"][..., 0]), mk(c["x1"], c["cond"][..., 1])
    tr = amb.Trainer(b, loss_fn, lr=1e-3)
    given = dict(t=c["t"], z=c["z"])
    first = tr.loss(batch0, batch1, **given)
    losses = [tr.step(batch0, batch1, **given) for _ in range(50)]
    last = tr.loss(batch0, batch1, **given)
    print(f"loss {first:.6f} -> {last:.6f} over 50 steps")
    assert losses[0] == first and np.isfinite(losses).all() and last < first - 0.05 * abs(first) and last < losses[0]
    # sync() yields a cPaiNN whose ti_painn_vloss on that batch is within the vloss bound of the trainer's last loss()
    assert tr.sync() is b
    val = loss_fn(batch0, batch1, b, **given)
    res = loss_fn.last
    eng = b.engine_for(A, m["src"], m["dst"], m["etype"], m["atom_ids"])
    v = eng.velocity_loss(c["x0"], c["x1"], c["cond"], returns=("b",), **pc.call_kw(c))
    bound = _ref_bound(dict(kind="standard", gamma="brownian", a=0.9), dict(x0=c["x0"], x1=c["x1"]), dict(t=c["t"], z=c["z"], bt_plus=v["b"][0], bt_minus=v["b"][1]))
    print(f"vloss of the synced model {val:.9f}, trainer {last:.9f}, bound {bound.sum() / (B * A):.3e}")
    assert val == res["mean"] and abs(val - last) <= bound.sum() / (B * A)
    sd = b.state_dict()
    assert set(sd) == {k for k, _ in c["spec"]} and not np.array_equal(sd["net.8.layers.0.phi.mlp.0.weight"], pc.split(c["flat"], c["spec"])["net.8.layers.0.phi.mlp.0.weight"])
    st = tr.state_dict()
    tr2 = amb.Trainer(amb.cPaiNN(n_features=F, score_layers=L), loss_fn, lr=1e-3).load_state_dict(st)
    assert tr2.step(batch0, batch1, **given) == tr.step(batch0, batch1, **given)


def test_latent_trainer_steps():
    ti = pkg()
    lat = import_module("thermodynamic-interpolation_amd.thermo.latent")
    F, L, A, B = 32, 1, 3, 5
    c = pc.make_case(1, F, L, A, B, kind="one_sided", center="batch", seed=8)
    m = c["model"]
    b = lat.cPaiNN(n_features=F, score_layers=L)
    b.load_state_dict(ti.weights.unflatten(c["flat"].astype(np.float32), c["spec"]))
    loss_fn = lat.losses.OneSidedVelocityLoss(lat.interpolants.OneSidedLinearInterpolant(), t_distr="beta")
    batch = SimpleNamespace(x0=c["x0"].reshape(B * A, 3), x1=c["x1"].reshape(B * A, 3), T=c["cond"].reshape(B * A).astype(np.int64),
                            atom_number=np.tile(m["atom_ids"], B).astype(np.int64), edge_index=ti.synthetic.batch_edge_index(m["src"], m["dst"], A, B),
                            edge_type=np.tile(m["etype"], B).astype(np.int64), batch=np.repeat(np.arange(B), A))
    tr = lat.Trainer(b, loss_fn, lr=1e-3)
    first = tr.loss(batch, seed=5, draw=2)
    assert first == pytest.approx(loss_fn(batch, b, seed=5, draw=2), abs=1e-5 * max(1.0, abs(first)))      # the same drawn t by either path
    losses = [tr.step(batch, seed=5, draw=2) for _ in range(10)]
    assert losses[0] == first and losses[-1] < first


# ------------------------------------------------------------------------------------------------ refusals that need a device
def test_workspace_budget_is_checked_before_any_work():
    ti = pkg()
    c = pc.fixture_case("painn_train_ambient", "brownian")
    tr = pc.make_trainer(c, max_workspace_bytes=1 << 20)
    need = tr.workspace_bytes(c["B"], "standard")
    assert need > 1 << 20 and tr.workspace_bytes(c["B"], "one_sided") < need
    for call in (tr.grad, tr.step):
        with pytest.raises(ti._lib.TiError) as ei:
            call(c["x0"], c["x1"], c["cond"], **pc.call_kw(c))
        assert ei.value.code == ti._lib.TI_E_UNSUPPORTED and str(need) in str(ei.value) and str(1 << 20) in str(ei.value)
    assert tr.state()["n_applied"] == 0
    # the header's formula
    F, L, A, E, B, nE = 32, 2, c["A"], c["model"]["src"].size, c["B"], 4
    Rn, Re = 2 * B * A, 2 * B * E
    want = (4 * (Re * (4 + F * (21 * L + 15)) + Rn * (F * (nE + 23 * L + 38) + 19) + 4 * F * max(Rn, Re) + 3 * B * A)
            + 4 * -(-max(Re, 3 * Rn) // 2048) * (8 * F * F + 11 * F) + 8 * (5 * F * -(-max(Rn, Re) // 2048) + 6 * B * A + B + max(3 * -(-B * A // 1024), -(-B // 1024), -(-tr.n_weights // 1024))))
    assert need == want
    small = pc.make_trainer(c)
    assert small.grad(c["x0"][:1], c["x1"][:1], c["cond"][:1], **dict(pc.call_kw(c), t=c["t"][:1], z=c["z"][:1]))["gnorm"] > 0.0


def test_wrong_kind_handles_are_refused_both_ways():
    ti = pkg()
    L_ = ti._lib.lib()
    c = pc.fixture_case("painn_train_ambient", "brownian")
    tr, eng = pc.make_trainer(c), _drift_engine(c)
    adw = ti.engine.AdwTrainer(32, 1, ti.weights.flatten_state_dict(ti.synthetic.adw_state_dict(32, 1), ti.weights.adw_param_spec(32, 1), dtype=np.float64))
    kw = pc.call_kw(c)
    for other in (eng, adw):                                  # a drift handle and an adw trainer into the molecule trainer's calls
        keep, tr.h = tr.h, other.h
        try:
            for call in (lambda: tr.grad(c["x0"], c["x1"], c["cond"], **kw), lambda: tr.step(c["x0"], c["x1"], c["cond"], **kw),
                         lambda: tr.apply(np.zeros(tr.n_weights)), tr.state, lambda: tr.set_lr(1e-3), lambda: tr.workspace_bytes(4)):
                with pytest.raises(ti._lib.TiError) as ei:
                    call()
                assert ei.value.code == ti._lib.TI_E_ARG and "not a painn trainer handle" in str(ei.value)
        finally:
            tr.h = keep
    x = np.zeros((1, c["A"], 3), np.float32)                  # the molecule trainer into the existing entry points
    vp = x.ctypes.data_as(C.c_void_p)
    assert L_.ti_painn_drift(tr.h, vp, C.c_float(0.5), vp, 1, vp, 0) == ti._lib.TI_E_ARG and "not a painn handle" in ti._lib.last_error()
    assert L_.ti_reserve(tr.h, 4) == ti._lib.TI_E_ARG
    assert L_.ti_adw_train_set_lr(tr.h, 1e-3) == ti._lib.TI_E_ARG and "not an adw trainer handle" in ti._lib.last_error()
    assert L_.ti_adw_drift(tr.h, vp, C.c_float(0.5), vp, vp, 1, vp, 0) == ti._lib.TI_E_ARG
    d = tr._vloss_desc("standard", "brownian", 1.0, "batch", None, "uniform", 0, 0, 0, 0)
    loss = np.zeros(1)
    assert L_.ti_painn_vloss(tr.h, C.byref(d), vp, vp, vp, None, None, 1, loss.ctypes.data_as(C.c_void_p), None, None, None, None, None, None, 0) == ti._lib.TI_E_ARG
