"""The molecule trainer on per-molecule graphs on the GPU (ti_painn_train_set_graphs): gradients against the reference's mixed-batch
fixtures and against the per-molecule restatement over the cells, the loss rows, the two identities and the other bit-for-bit
properties, the Python path down to the driver, and the refusals that need a trainer handle."""
import ctypes as C
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import painn_train_cases as pc
import painn_train_graphs_cases as gc
from conftest import load_golden, pkg
from test_gpu_painn_train import _check_grad
from test_gpu_vloss import _ref_bound

pytestmark = pytest.mark.gpu

FIXTURES = ["painn_train_graphs_ambient", "painn_train_graphs_latent"]
_REF = {}


def _reference(c):
    """(rows, mean, g64, g32, drift) of the restatement, computed once per case and shared"""
    if c["name"] not in _REF:
        rows, mean, g64, drift = gc.reference(c)
        _, _, g32, _ = gc.reference(c, torch.float32)
        _REF[c["name"]] = (rows, mean, g64, g32, drift)
    return _REF[c["name"]]


def _check_loss(c, r, rows64, mean64, drift):
    """Loss rows and mean against fp64 within the bound of tests/test_gpu_vloss.py, stated in the fp64 drift on the real entries (the
    pads hold zeros in every array of the bound, so they add nothing to it); the mean is the sum of the rows over N"""
    s = dict(kind=c["lk"]["kind"], gamma=c["lk"]["gamma"], a=c["lk"]["a"])
    z = None if c["z"] is None else gc.zero_pads(c, c["z"])
    bound = _ref_bound(s, dict(x0=gc.zero_pads(c, c["x0"]), x1=gc.zero_pads(c, c["x1"])), dict(t=c["t"], z=z, bt_plus=drift[0], bt_minus=drift[-1]))
    print(f"   loss against fp64: max |dl| / bound {np.max(np.abs(r['loss'] - rows64) / bound):.3e}; mean {r['mean']:.9f} (fp64 {mean64:.9f})")
    assert (np.abs(r["loss"] - rows64) <= bound).all()
    assert abs(r["mean"] - mean64) <= bound.sum() / c["N"]
    assert r["mean"] == pytest.approx(r["loss"].sum() / c["N"], rel=1e-14)


def _same(p, q):
    return np.array_equal(p["grad"], q["grad"]) and np.array_equal(np.asarray(p["loss"]), np.asarray(q["loss"])) and p["mean"] == q["mean"] and p["gnorm"] == q["gnorm"]


def _grad(tr, c):
    return tr.grad(c["x0"], c["x1"], c["cond"], **pc.call_kw(c))


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("name", FIXTURES)
def test_gradients_against_the_reference_on_a_mixed_batch(name):
    """Per tensor, rel-L2 against the reference's fp64 gradient <= max(1e-5, 3 x the reference's own float32 distance)"""
    c = gc.fixture_case(name)
    r = _grad(gc.make_trainer(c), c)
    print(f"{name}: mean {r['mean']:.9f} (reference {float(c['mean64']):.9f})")
    assert all(d >= 0.0 for d in c["d32"].values())
    _check_grad(c, r, c["g64"], {k: max(1e-5, 3.0 * d) for k, d in c["d32"].items()})
    _, _, _, _, drift = _reference(c)
    _check_loss(c, r, c["rows64"], float(c["mean64"]), drift)


@pytest.mark.parametrize("name", gc.CELL_IDS)
def test_gradient_cells(name):
    """A cell against the per-molecule restatement: every tensor under max(1e-5, 3 x the float32 restatement's distance), the zero
    pattern, the norm, the loss rows and the mean over N"""
    c = gc.graph_case(name)
    rows, mean, g64, g32, drift = _reference(c)
    r = _grad(gc.make_trainer(c), c)
    bars = {k: bar for k, _, bar in pc.tensor_errors(g32, g64, g32) if bar > 0.0}
    _check_grad(c, r, g64, bars)
    _check_loss(c, r, rows, mean, drift)
    if name == "single":                                      # the one-atom molecule: a zero drift, so its loss row is exactly zero
        b = int(np.flatnonzero(c["n_atoms"] == 1)[0])
        assert rows[b] == 0.0 and r["loss"][b] == 0.0


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("kind,center", [("standard", "batch"), ("standard", "molecule"), ("one_sided", "none")])
def test_a_full_table_is_the_call_without_a_table(kind, center):
    """Identity (a): n_atoms = A, every template bit set, pair_type None -- the outputs of grad, and the state after steps"""
    c = pc.make_case(0, 32, 2, 7, 5, tpl="sparse", kind=kind, gamma="sin2", center=center, seed=3)
    kw = pc.call_kw(c)
    plain, table = pc.make_trainer(c, lr=1e-3), pc.make_trainer(c, lr=1e-3)
    A, B = c["A"], c["B"]
    full = np.zeros((B, A), np.uint32)
    np.bitwise_or.at(full, (slice(None), c["model"]["dst"]), np.uint32(1) << c["model"]["src"].astype(np.uint32))
    table.set_graphs(np.full(B, A, np.int32), full, None)
    a, b = plain.grad(c["x0"], c["x1"], c["cond"], **kw), table.grad(c["x0"], c["x1"], c["cond"], **kw)
    assert _same(a, b) and a["gnorm"] > 0.0
    drawn = dict(kw, t=None, z=None, seed=11, traj_offset=(1 << 32) + 5, draw=3)             # and with t and z drawn
    assert _same(plain.grad(c["x0"], c["x1"], c["cond"], **drawn), table.grad(c["x0"], c["x1"], c["cond"], **drawn))
    for k in range(3):
        assert plain.step(c["x0"], c["x1"], c["cond"], **kw) == table.step(c["x0"], c["x1"], c["cond"], **kw)
    sa, sb = plain.state(), table.state()
    assert all(np.array_equal(sa[q], sb[q]) for q in "wmv") and sa["n_applied"] == sb["n_applied"] == 3
    table.set_graphs(None, None, None)                        # cleared: the plain call again; all-None masks are a full table too
    assert _same(plain.grad(c["x0"], c["x1"], c["cond"], **kw), table.grad(c["x0"], c["x1"], c["cond"], **kw))
    table.set_graphs(np.full(B, A, np.int32))
    assert _same(plain.grad(c["x0"], c["x1"], c["cond"], **kw), table.grad(c["x0"], c["x1"], c["cond"], **kw))


@pytest.mark.parametrize("name", ["standard", "one_sided-molecule", "one_sided-none"])
def test_results_do_not_depend_on_the_pads_or_the_call(name):
    """Pad entries of x0, x1, cond and z poisoned with several finite values; the same call twice; host against device pointers;
    the same call after a larger one"""
    c = gc.graph_case(name)
    tr = gc.make_trainer(c)
    a = _grad(tr, c)
    assert np.isfinite(a["grad"]).all() and a["gnorm"] > 0.0 and _same(a, _grad(tr, c))
    for value in (7.5, -3.0e4, 1.0e30):
        assert _same(a, _grad(tr, gc.poisoned(c, value))), value
    dev = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()
    kw = pc.call_kw(c)
    d = tr.grad(dev(c["x0"]), dev(c["x1"]), dev(c["cond"]), **dict(kw, t=dev(kw["t"]), z=dev(kw["z"])))
    d["loss"] = d["loss"].cpu().numpy()
    assert _same(a, d)
    tr.set_graphs(dev(c["n_atoms"]), dev(c["mask"].view(np.int32)), dev(c["pair_type"]))     # the table from device arrays
    assert _same(a, _grad(tr, c))
    wide = pc.make_case(c["model"]["variant"], 32, 2, c["A"], 23, tpl="full", kind=c["lk"]["kind"], gamma=c["lk"]["gamma"], a=c["lk"]["a"],
                        center=c["center"], seed=4)
    tr.set_graphs(None, None, None)                           # a larger call, without a table, on the same trainer
    tr.grad(wide["x0"], wide["x1"], wide["cond"], **pc.call_kw(wide))
    tr.set_graphs(c["n_atoms"], c["mask"], c["pair_type"])
    assert _same(a, _grad(tr, c))


def _pool(variant, kind, center, n0=7, n1=9, A=4, B=3, steps=3, seed=2):
    """Two resident sets with temperatures, a table of n0 graphs, [steps, B] indices"""
    c = pc.make_case(variant, 32, 1, A, n1, tpl="full", kind=kind, gamma="sin2", center=center, seed=seed)
    rs = np.random.RandomState(90 + seed)
    c["set0"], c["set1"] = np.ascontiguousarray(c["x0"][:n0]), np.ascontiguousarray(c["x1"])
    c["temp0"] = (300.0 + 100.0 * (np.arange(n0) % 8)).astype(np.float32)
    c["temp1"] = (300.0 + 100.0 * (np.arange(n1) % 6)).astype(np.float32)
    c["idx0"] = np.stack([rs.permutation(n0)[:B] for _ in range(steps)]).astype(np.int64)
    c["idx1"] = np.stack([rs.permutation(n1)[:B] for _ in range(steps)]).astype(np.int64)
    c["idx0"][1, 2] = c["idx0"][1, 0]                         # a table row twice in one minibatch
    c["tab_n"] = rs.randint(1, A + 1, n0).astype(np.int32)
    c["tab_n"][:2] = (A, 2)
    c["tab_mask"], c["tab_pt"] = gc._random_graphs(rs, n0, A, c["tab_n"])
    c["ncond"] = {0: 2, 1: 1, 2: 0}[variant]
    c["kw"] = dict(kind=kind, gamma="sin2", a=1.0, center=center, t_distr="beta_half", seed=77, traj_offset=(1 << 32) + 9)
    return c


def _cond(c, r0, r1):
    if c["ncond"] == 0:
        return None
    cols = [c["temp0"][r0], c["temp1"][r1]] if c["ncond"] == 2 else [c["temp1"][r1]]
    return np.ascontiguousarray(np.stack([np.repeat(v[:, None], c["A"], axis=1) for v in cols], axis=-1).astype(np.float32))


def _temps(c):
    return (c["temp0"] if c["ncond"] == 2 else None), (c["temp1"] if c["ncond"] >= 1 else None)


def _same_state(a, b):
    sa, sb = a.state(), b.state()
    return all(np.array_equal(sa[q], sb[q]) for q in "wmv") and sa["n_applied"] == sb["n_applied"] and sa["n_skipped"] == sb["n_skipped"]


@pytest.mark.parametrize("variant,kind,center", [(0, "standard", "batch"), (1, "one_sided", "molecule")])
def test_steps_equal_the_loop_of_set_graphs_and_step(variant, kind, center):
    """Identity (b): a many-step call with the table of set 0 in force, from host and from device sets and indices, against the loop
    of ti_painn_train_set_graphs on the gathered rows and ti_painn_train_step; then update = 0 against ti_painn_train_grad's mean"""
    c = _pool(variant, kind, center)
    DRAW, steps = 40, c["idx0"].shape[0]
    t0, t1 = _temps(c)
    host, loop, dev = (pc.make_trainer(c, lr=1e-3) for _ in range(3))
    for tr in (host, dev):
        tr.set_graphs(c["tab_n"], c["tab_mask"], c["tab_pt"])
    lh, sh = host.steps(c["set0"], c["set1"], t0, t1, c["idx0"], c["idx1"], draw=DRAW, **c["kw"])
    cu = lambda v: None if v is None else torch.from_numpy(v).cuda()
    ld, sd = dev.steps(cu(c["set0"]), cu(c["set1"]), cu(t0), cu(t1), cu(c["idx0"]), cu(c["idx1"]), draw=DRAW, **c["kw"])
    ll = []
    for k in range(steps):
        r0, r1 = c["idx0"][k], c["idx1"][k]
        loop.set_graphs(c["tab_n"][r0], c["tab_mask"][r0], c["tab_pt"][r0])
        ll.append(loop.step(np.ascontiguousarray(c["set0"][r0]), np.ascontiguousarray(c["set1"][r1]), _cond(c, r0, r1), draw=DRAW + k, **c["kw"])[0])
    print(f"losses {lh}")
    assert np.isfinite(lh).all() and sh == sd == 0 and np.array_equal(lh, ll) and np.array_equal(lh, ld)
    assert _same_state(host, loop) and _same_state(host, dev) and host.state()["n_applied"] == steps
    # forward only: the losses of the same minibatches at the current weights are ti_painn_train_grad's means
    before = host.state()
    lf, sf = host.steps(c["set0"], c["set1"], t0, t1, c["idx0"], c["idx1"], draw=DRAW, update=False, **c["kw"])
    for k in range(steps):
        r0, r1 = c["idx0"][k], c["idx1"][k]
        loop.set_graphs(c["tab_n"][r0], c["tab_mask"][r0], c["tab_pt"][r0])
        g = loop.grad(np.ascontiguousarray(c["set0"][r0]), np.ascontiguousarray(c["set1"][r1]), _cond(c, r0, r1), draw=DRAW + k, **c["kw"])
        assert lf[k] == g["mean"], k
    assert sf == 0 and all(np.array_equal(before[q], host.state()[q]) for q in "wmv")
    # without indices: rows 0..B-1 of the table
    B = c["idx0"].shape[1]
    l1, _ = host.steps(c["set0"], c["set1"], t0, t1, batch=B, draw=DRAW + 9, **c["kw"])
    r = np.arange(B)
    loop.set_graphs(c["tab_n"][:B], c["tab_mask"][:B], c["tab_pt"][:B])
    m1, _ = loop.step(np.ascontiguousarray(c["set0"][:B]), np.ascontiguousarray(c["set1"][:B]), _cond(c, r, r), draw=DRAW + 9, **c["kw"])
    assert l1[0] == m1 and _same_state(host, loop)


# ------------------------------------------------------------------------------------------------ the Python path
def test_per_molecule_trainer_steps_on_a_collated_mixed_batch():
    """thermo.ambient.Trainer with batches='per_molecule': one step on the reference-style mixed batch of the fixture is the engine
    call on the padded arrays with the batch's graphs set"""
    ti = pkg()
    amb = import_module("thermodynamic-interpolation_amd.thermo.ambient")
    c = gc.fixture_case("painn_train_graphs_ambient")
    g = load_golden("painn_train_graphs_ambient")
    ids = np.concatenate([np.arange(n) for n in g["n_atoms"]]).astype(np.int64)
    mk = lambda x, T: SimpleNamespace(x=x, T=T, atoms=ids, edge_index=g["edge_index"], edge_type=g["edge_type"], batch=g["batch"])
    batch0, batch1 = mk(g["x0"], g["cond"][:, 0]), mk(g["x1"], g["cond"][:, 1])
    b = amb.cPaiNN(n_features=c["model"]["F"], score_layers=c["model"]["L"], temp_length=c["model"]["temp_length"])
    b.load_state_dict(ti.weights.unflatten(c["flat"], c["spec"]))
    loss_fn = amb.losses.StandardVelocityLoss(amb.interpolants.LinearInterpolant(a=c["lk"]["a"], gamma=c["lk"]["gamma"]))
    tr = amb.Trainer(b, loss_fn, lr=1e-3).with_batches("per_molecule", max_atoms=c["A"])
    eng = gc.make_trainer(c, lr=1e-3)
    given = dict(t=g["t"], z=g["z"])
    want = eng.grad(c["x0"], c["x1"], c["cond"], **pc.call_kw(c))["mean"]
    assert tr.loss(batch0, batch1, **given) == want
    assert tr.step(batch0, batch1, **given) == eng.step(c["x0"], c["x1"], c["cond"], **pc.call_kw(c))[0] == want
    assert _same_state(tr.engine, eng) and tr.engine.state()["n_applied"] == 1
    per_node_t = np.repeat(g["t"], g["n_atoms"])
    assert tr.loss(batch0, batch1, t=per_node_t, z=g["z"]) == eng.grad(c["x0"], c["x1"], c["cond"], **pc.call_kw(c))["mean"]
    with pytest.raises(RuntimeError):
        tr.with_batches("uniform")


def _template(m, A, n=2):
    ti = pkg()
    return SimpleNamespace(x=np.zeros((n * A, 3), np.float32), T=np.full(n * A, 300.0, np.float32), atoms=np.tile(m["atom_ids"], n).astype(np.int64),
                           edge_index=ti.synthetic.batch_edge_index(m["src"], m["dst"], A, n), edge_type=np.tile(m["etype"], n).astype(np.int64),
                           batch=np.repeat(np.arange(n), A))


def test_fit_with_masks_equals_the_loop_and_the_driver_trains_on_radius_graphs(tmp_path):
    ti = pkg()
    amb = import_module("thermodynamic-interpolation_amd.thermo.ambient")
    adw = import_module("thermodynamic-interpolation_amd.thermo.adw")
    c = _pool(0, "standard", "batch", n0=11, n1=13)
    A, B, m = c["A"], 3, c["model"]
    tpl = _template(m, A)
    b = amb.cPaiNN(n_features=32, score_layers=1)
    b.load_state_dict(ti.weights.unflatten(c["flat"], c["spec"]))
    loss_fn = amb.losses.StandardVelocityLoss(amb.interpolants.LinearInterpolant(a=1.0, gamma="sin2"))
    tr = amb.Trainer(b, loss_fn, lr=1e-3)
    masks = gc._random_graphs(np.random.RandomState(5), 11, A, None)[0]
    sets = (c["set0"], c["temp0"], c["set1"], c["temp1"])
    losses, skipped = tr.fit(*sets, B, 3, [3, 0], draw=4, noise_seed=3, template_batch=tpl, masks=masks)
    ev = tr.evaluate(*sets, B, 3, [3, 0], draw=4, noise_seed=3, masks=masks)
    rng = np.random.default_rng([3, 0])
    i0, i1 = adw.minibatch_indices(11, B, 3, rng), adw.minibatch_indices(13, B, 3, rng)
    loop = pc.make_trainer(c, lr=1e-3)
    kw = dict(kind="standard", gamma="sin2", a=1.0, center="batch", t_distr="uniform", seed=3)
    want = []
    for k in range(3):
        loop.set_graphs(None, masks[i0[k]], None)
        want.append(loop.step(np.ascontiguousarray(c["set0"][i0[k]]), np.ascontiguousarray(c["set1"][i1[k]]), _cond(c, i0[k], i1[k]), draw=4 + k, **kw)[0])
    assert skipped == 0 and np.array_equal(losses, want) and _same_state(tr.engine, loop)
    assert ev.shape == (3,) and np.isfinite(ev).all() and not np.array_equal(ev, losses)
    plain, _ = amb.Trainer(amb.cPaiNN(n_features=32, score_layers=1).load_state_dict(ti.weights.unflatten(c["flat"], c["spec"])), loss_fn, lr=1e-3).fit(
        *sets, B, 3, [3, 0], draw=4, noise_seed=3, template_batch=tpl)
    assert not np.array_equal(plain, losses)                  # the masks do something
    with pytest.raises(ValueError, match="masks"):
        tr.fit(*sets, B, 3, [3, 0], masks=masks[:5])

    # the driver: two epochs on radius graphs, files, and a resumed run against a whole one, bit for bit
    def config(n_epochs, name, **extra):
        return SimpleNamespace(n_features=32, score_layers=1, batch_size=B, n_epochs=n_epochs, learning_rate=1e-3, weight_decay=0.0, a=1.0, gamma="sin2",
                               t_distr="uniform", seed=5, align=False, model_save_path=str(tmp_path), model_save_name=name, **extra)
    set0, set1 = (c["set0"], c["temp0"]), (c["set1"], c["temp1"])
    d = np.linalg.norm(c["set0"][:, :, None] - c["set0"][:, None], axis=-1)[:, ~np.eye(A, dtype=bool)]
    cutoff = float(np.quantile(d, 0.6))
    rg = dict(radius_graphs=True, cutoff=cutoff)
    log = ti.drivers.train_ambient(config(1, "run", **rg), set0, set1, tpl)
    out = os.path.join(str(tmp_path), "run")
    assert all(v.shape == (1,) for v in log.values()) and np.isfinite(log["train_loss"]).all() and (log["skipped"] == 0).all()
    assert os.path.exists(os.path.join(out, "run_0_weights.npz")) and os.path.exists(os.path.join(out, "run_best0_weights.npz"))
    resumed = ti.drivers.train_ambient(config(2, "run", **rg), set0, set1, tpl, resume=True)
    whole = ti.drivers.train_ambient(config(2, "whole", **rg), set0, set1, tpl)
    assert all(np.array_equal(resumed[k], whole[k]) for k in whole) and all(v.shape == (2,) for v in whole.values())
    with np.load(os.path.join(out, "run_1_weights.npz")) as p, np.load(os.path.join(str(tmp_path), "whole", "whole_1_weights.npz")) as q:
        assert set(p.files) == set(q.files) and all(np.array_equal(p[k], q[k]) for k in p.files)
    without = ti.drivers.train_ambient(config(2, "plain"), set0, set1, tpl)
    assert not np.array_equal(without["train_loss"], whole["train_loss"])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_with_a_trainer_handle():
    """ti_painn_train_set_graphs's checks behind the handle check, in their order; the table against B and n0; drawn noise with a
    table; the drift's graph calls keep refusing a trainer; the version"""
    ti = pkg()
    L_ = ti._lib.lib()
    E_ARG, E_UNS = ti._lib.TI_E_ARG, ti._lib.TI_E_UNSUPPORTED
    c = gc.graph_case("one_sided-batch")
    A, B = c["A"], c["B"]
    tr = pc.make_trainer(c)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n_bad, n_ok = np.asarray([A, 0, A + 1], np.int32), np.asarray(c["n_atoms"], np.int32)
    t_bad = np.full((B, A, A), 4, np.uint8)
    err = lambda: L_.ti_last_error().decode()
    sg = L_.ti_painn_train_set_graphs
    assert sg(tr.h, vp(n_bad), None, vp(t_bad), 0, 9) == E_ARG and "n < 1" in err()                     # n before the counts, the types and mem
    assert sg(tr.h, vp(n_bad), None, vp(t_bad), B, 9) == E_ARG and "n_atoms[1] = 0" in err()            # counts before the types and mem
    assert sg(tr.h, vp(n_ok), None, vp(t_bad), B, 9) == E_ARG and "pair_type above 3" in err()          # types before mem
    assert sg(tr.h, vp(n_ok), None, None, B, 9) == E_ARG and "unknown mem" in err()
    dn, dt = torch.from_numpy(n_bad).cuda(), torch.from_numpy(t_bad).cuda()                               # device arrays: after their copy
    assert sg(tr.h, C.c_void_p(dn.data_ptr()), None, None, B, 1) == E_ARG and "n_atoms[1] = 0" in err()
    assert sg(tr.h, None, None, C.c_void_p(dt.data_ptr()), B, 1) == E_ARG and "pair_type above 3" in err()
    r0 = _grad(tr, c)                                         # nothing was set by the refused calls: the plain call
    assert _same(r0, _grad(pc.make_trainer(c), c))
    tr.set_graphs(c["n_atoms"], c["mask"], c["pair_type"])
    kw = pc.call_kw(c)
    for call in (tr.grad, tr.step):                           # n != B
        with pytest.raises(ti._lib.TiError) as ei:
            call(c["x0"][:2], c["x1"][:2], c["cond"][:2], **dict(kw, t=c["t"][:2]))
        assert ei.value.code == E_ARG and "rows" in str(ei.value)
    assert tr.state()["n_applied"] == 0
    x1, t1 = np.concatenate([c["x1"], c["x1"]]), np.full(2 * B, 300.0, np.float32)
    skw = dict(kind="one_sided", gamma="brownian", a=1.0, center="batch", t_distr="uniform", seed=1)
    with pytest.raises(ti._lib.TiError) as ei:                # n != n0
        tr.steps(x1, x1, None, t1, batch=B, **skw)
    assert ei.value.code == E_ARG and "n0" in str(ei.value)
    for noise in ("drawn", "aligned"):
        with pytest.raises(ti._lib.TiError) as ei:
            tr.steps(None, c["x1"], None, t1[:B], batch=B, noise=noise, **skw)
        assert ei.value.code == E_UNS and "ti_painn_train_set_graphs" in str(ei.value)
    l, _ = tr.steps(c["x0"], c["x1"], None, t1[:B], batch=B, update=False, **skw)                       # n == n0 == B: served
    assert np.isfinite(l).all()
    tr.set_graphs()                                           # cleared: drawn noise is served again
    l, _ = tr.steps(None, c["x1"], None, t1[:B], batch=B, noise="drawn", update=False, **skw)
    assert np.isfinite(l).all()
    m = np.zeros((B, A), np.uint32)
    assert L_.ti_painn_set_edge_mask(tr.h, vp(m), B, 0) == E_ARG and "not a painn handle" in err()
    assert L_.ti_painn_set_molecules(tr.h, vp(n_ok), None, None, B, 0) == E_ARG and "not a painn handle" in err()
    eng = ti.engine.PainnEngine(c["model"]["variant"], 32, 2, A, c["model"]["src"], c["model"]["dst"], c["model"]["etype"], c["model"]["atom_ids"],
                                c["flat"].astype(np.float32))
    assert sg(eng.h, vp(n_ok), None, None, B, 0) == E_ARG and "not a painn trainer handle" in err()
    assert L_.ti_version() == 5
