"""The molecule trainer without a GPU: the torch restatement of cPaiNN (tests/painn_train_torch.py) against the reference's own
autograd gradients, the restated optimiser against three reference steps, the float32 restatement over the GPU test's shape matrix,
every refusal that is raised before the device in its stated order, and the Python signatures."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import adw_train_numpy as an
import painn_train_cases as pc
from conftest import load_golden, pkg


@pytest.fixture(scope="module")
def lib():
    ti = pkg()
    ti.build.build()
    return ti._lib.lib()


def test_sources_and_symbols_are_listed(lib):
    ti = pkg()
    assert "painn_train_kernels.hip" in ti.build.SOURCES and "api_painn_train.hip" in ti.build.SOURCES and "painn_train.hpp" in ti.build.HEADERS
    for n in ("ti_painn_trainer_create", "ti_painn_train_grad", "ti_painn_train_apply", "ti_painn_train_step", "ti_painn_train_get_state",
              "ti_painn_train_set_state", "ti_painn_train_set_lr", "ti_painn_train_workspace_bytes"):
        assert n in ti._lib.ABI_SYMBOLS and hasattr(lib, n)


# ------------------------------------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("name,case", pc.FIXTURE_CASES)
def test_restatement_reproduces_the_reference_gradients(name, case):
    """fp64 restatement against the fixtures' fp64 gradients: per tensor <= 1e-10 rel-L2; what the reference leaves exactly zero is
    exactly zero; the loss rows and the mean to fp64 round-off."""
    c = pc.fixture_case(name, case)
    rows, mean, g = pc.reference(c)
    errs = pc.tensor_errors(g, c["g64"])
    worst = max(errs, key=lambda r: r[1])
    print(f"{name} {case}: worst tensor {worst[0]} {worst[1]:.3e}")
    for k, e, _ in errs:
        assert e <= 1e-10, (k, e)
    assert pc.zero_violations(g, c["g64"]) == []
    assert any(np.any(r == 0.0) for r in c["g64"].values())          # the fixture does hold exact zeros (the last layer's de chunk)
    assert np.max(np.abs(rows - c["rows64"])) <= 1e-12 * np.max(np.abs(c["rows64"]))
    assert abs(mean - float(c["mean64"])) <= 1e-12 * abs(float(c["mean64"]))


def test_restated_optimiser_reaches_the_three_reference_steps():
    """clip_grad_norm_ 1 + Adam lr 1e-4 restated (tests/adw_train_numpy.py) from the reference's gradient bits of every step reaches
    the reference's weights after three steps within 16 k 2^-53 (|p| + lr); the clip is active in every step."""
    c = pc.fixture_case("painn_train_ambient", "brownian")
    g, st = load_golden("painn_train_ambient"), load_golden("painn_train_ambient_steps")
    lr = float(g["steps::lr"])
    flat = lambda d: np.concatenate([np.asarray(d[k], np.float64).ravel() for k, _ in c["spec"]])
    grads = [flat(c["g64"])] + [flat({k: st[f"steps::{i}::g::{k}"] for k, _ in c["spec"]}) for i in (1, 2)]
    assert all(float(g[f"steps::{i}::gnorm"]) > 1.0 for i in range(3))
    opt = an.Adam(c["flat"], lr=lr, max_grad_norm=1.0)
    for gr in grads:
        assert not opt.step(gr)
    want = flat({k: g[f"steps::w::{k}"] for k, _ in c["spec"]})
    ratio = np.max(np.abs(opt.w - want) / an.adam_bound(want, lr, 3))
    print(f"three steps: {ratio:.3f} of the bound; moved by {np.max(np.abs(want - c['flat'])):.2e}")
    assert ratio <= 1.0
    assert np.max(np.abs(want - c["flat"])) > 0.5 * lr


@pytest.mark.parametrize("cell", pc.MATRIX + pc.EDGE_MATRIX, ids=pc.MATRIX_IDS + pc.EDGE_IDS)
def test_float32_restatement_stays_inside_a_third_of_the_bar(cell):
    """The inputs of the GPU shape matrix are kept only where the plain float32 model stays below 1e-5 / 3 per tensor, so that the
    1e-5 floor decides there and not the luck of a cancelling sum.  In the cells of FLOAT32_DECIDES the tensors
    above it are the `v.linear.weight` ones alone, and they stay below 1e-5 (the bar there is 3 x this distance).  The edge cells
    follow the same rule; in those of EDGE_FLOAT32_DECIDES the tensors above a third are among the recorded ones, every recorded one
    is close to a third or above it, and every tensor stays below 1e-5."""
    c = pc.matrix_case(cell)
    _, _, g64 = pc.reference(c)
    _, _, g32 = pc.reference(c, torch.float32)
    errs = pc.tensor_errors(g32, g64)
    worst = max(errs, key=lambda r: r[1])
    print(f"{cell}: float32 restatement worst {worst[0]} {worst[1]:.3e}")
    edge = cell in pc.EDGE_MATRIX
    if edge and pc.EDGE_MATRIX.index(cell) in pc.EDGE_FLOAT32_DECIDES:
        recorded = pc.EDGE_FLOAT32_DECIDES[pc.EDGE_MATRIX.index(cell)]
        now = {k: e for k, e, _ in errs}
        over = {k for k, e in now.items() if e > 1e-5 / 3}
        for k in sorted(over | set(recorded)):
            print(f"   {k}: {now[k]:.3e} (recorded {recorded.get(k, float('nan')):.3e})")
        # the float32 restatement is not the same bits on every host (pc.EDGE_FLOAT32_DECIDES has the spread that was measured), so the
        # recorded set reaches that spread below a third: what is above a third here is recorded, and nothing is recorded that is
        # not close to a third here
        assert over <= set(recorded), sorted(over - set(recorded))
        assert all(now[k] >= 1e-5 / 3 / pc.EDGE_HOST_SPREAD ** 2 for k in recorded)
        assert worst[1] <= 1e-5 and all(d <= 1e-5 for d in recorded.values())
    elif not edge and pc.MATRIX.index(cell) in pc.FLOAT32_DECIDES:
        assert all(e <= 1e-5 / 3 or (k.endswith("v.linear.weight") and e <= 1e-5) for k, e, _ in errs)
    else:
        assert worst[1] <= 1e-5 / 3
    et = c["model"]["etype"]
    assert c["A"] == 2 or set(et.tolist()) == {0, 1, 2, 3}
    if cell[5] == "sparse":
        indeg = np.bincount(c["model"]["dst"], minlength=c["A"])
        assert indeg[0] == 0 and len(set(indeg.tolist())) > (2 if c["A"] > 3 else 1)


# ------------------------------------------------------------------------------------------------ refusals before the device
def _create(lib, ti, *, F=32, L=1, A=3, E=6, variant=0, n_types=25, precision=0, n_w=None, td="ok", src=None, ids=None, weights=True):
    d = ti._lib.PainnDesc(variant, F, L, n_types, A, E, 100.0, 10.0, 10.0, 650.0, 700.0, precision)
    n = ti.weights.n_params(ti.weights.painn_param_spec(min(max(variant, 0), 2), F if F in (32, 64, 128, 256) else 32, max(L, 1), max(n_types, 1)))
    w = np.zeros(n if n_w is None else n_w, np.float64)
    s, dd, et = (np.ascontiguousarray(a, np.int32) for a in ti.synthetic.fully_connected_template(3))
    if src is not None:
        s = np.ascontiguousarray(src, np.int32)
    ai = np.ascontiguousarray(np.arange(max(A, 1)) if ids is None else ids, np.int32)
    tdesc = ti._lib.PainnTrainDesc(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0) if td == "ok" else td
    h = lib.ti_painn_trainer_create(C.byref(d), w.ctypes.data_as(C.POINTER(C.c_double)) if weights else None, w.size, ti._lib.iptr(s), ti._lib.iptr(dd),
                                    ti._lib.iptr(et), ti._lib.iptr(ai), C.byref(tdesc) if tdesc is not None else None, 0)
    return h, lib.ti_last_error().decode()


def test_create_refusals_come_before_the_device_in_order(lib):
    ti = pkg()
    T = ti._lib.PainnTrainDesc
    cases = [(dict(weights=False), "NULL argument"), (dict(F=48), "n_features"), (dict(L=0), "n_layers"), (dict(A=40), "n_atoms"),
             (dict(E=-1), "edge arrays"), (dict(variant=3), "unknown variant"), (dict(n_types=0), "n_types"), (dict(precision=7), "unknown precision"),
             (dict(src=[0, 0, 1, 1, 2, 9]), "edge index"), (dict(ids=[0, 1, 99]), "atom id"), (dict(n_w=5), "weight count"),
             # each of the following is wrong in what comes later too: the earlier check answers
             (dict(precision=1, E=0, td=None), "TI_PREC_F32"), (dict(E=0, td=None), "n_edges == 0"), (dict(td=None), "train desc is NULL"),
             (dict(td=T(0.0, 0.9, 0.999, 1e-8, 0.0, 1.0, 0)), "lr"), (dict(td=T(1e-3, 1.0, 0.999, 1e-8, 0.0, 1.0, 0)), "beta1"),
             (dict(td=T(1e-3, 0.9, 0.999, 0.0, 0.0, 1.0, 0)), "eps"), (dict(td=T(1e-3, 0.9, 0.999, 1e-8, -1.0, 1.0, 0)), "weight_decay"),
             (dict(td=T(1e-3, 0.9, 0.999, 1e-8, 0.0, float("nan"), 0)), "max_grad_norm")]
    for kw, word in cases:
        h, msg = _create(lib, ti, **kw)
        assert not h and word in msg, (kw, msg)
    # a complete, valid call reaches the device: on a machine without one that is what fails
    if lib.ti_device_count() == 0:
        h, msg = _create(lib, ti)
        assert not h and "HIP" in msg


def test_call_refusals_follow_the_velocity_loss_order(lib):
    """vloss_check in its order, then a NULL buffer, then the handle (the workspace check needs a trainer: tests/test_gpu_painn_train.py)"""
    ti = pkg()
    E = ti._lib.TI_E_ARG
    D = lambda **kw: ti._lib.VlossDesc(**{**dict(kind=0, gamma=0, a=1.0, center=0, t_dist=1, seed=0, traj_offset=0, draw=0, n_tbins=0), **kw})
    x = np.zeros(18, np.float32)
    tv = np.full(2, 0.5, np.float32)
    xp, tp = x.ctypes.data_as(C.c_void_p), tv.ctypes.data_as(C.c_void_p)

    def grad(desc, B=2, mem=0, x0=True, t=None, z=None):
        return lib.ti_painn_train_grad(None, C.byref(desc) if desc is not None else None, xp if x0 else None, xp, None, t, z, B, None, None, None, None, mem)

    def step(desc, B=2, mem=0, x0=True, t=None, z=None):
        return lib.ti_painn_train_step(None, C.byref(desc) if desc is not None else None, xp if x0 else None, xp, None, t, z, B, None, None, mem)

    for fn in (grad, step):
        for word, kw in (("desc is NULL", dict(desc=None)), ("loss kind", dict(desc=D(kind=5), B=0)), ("gamma kind", dict(desc=D(gamma=9), B=0)),
                         ("center mode", dict(desc=D(center=7), B=0)), ("time distribution", dict(desc=D(t_dist=9), B=0)),
                         ("parameter a", dict(desc=D(a=0.0), B=0)), ("n_tbins", dict(desc=D(n_tbins=-1), B=0)), ("B < 1", dict(desc=D(), B=0, mem=9)),
                         ("unknown mem", dict(desc=D(), mem=9, x0=False)), ("z must be NULL", dict(desc=D(kind=1), z=xp, x0=False)),
                         ("GIVEN needs t", dict(desc=D(t_dist=0), x0=False)), ("t must be NULL", dict(desc=D(), t=tp, x0=False)),
                         ("NULL buffer", dict(desc=D(), x0=False)), ("not a painn trainer handle", dict(desc=D()))):
            assert fn(**kw) == E and word in lib.ti_last_error().decode(), (fn.__name__, word, lib.ti_last_error().decode())
    g = np.zeros(4)
    assert lib.ti_painn_train_apply(None, None, None) == E and "NULL buffer" in lib.ti_last_error().decode()
    assert lib.ti_painn_train_apply(None, g.ctypes.data_as(C.POINTER(C.c_double)), None) == E and "trainer handle" in lib.ti_last_error().decode()
    assert lib.ti_painn_train_set_state(None, None, None, None, -1) == E and "n_applied" in lib.ti_last_error().decode()
    assert lib.ti_painn_train_set_lr(None, 0.0) == E and "lr" in lib.ti_last_error().decode()
    assert lib.ti_painn_train_get_state(None, None, None, None, None, None) == E
    assert lib.ti_painn_train_workspace_bytes(None, 0, 0) == E and lib.ti_painn_train_workspace_bytes(None, 4, 0) == E


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_signatures():
    ti = pkg()
    from importlib import import_module
    sig = lambda f: list(inspect.signature(f).parameters)
    PT = ti.engine.PainnTrainer
    assert sig(PT.__init__)[:10] == ["self", "variant", "F", "L", "A", "edge_src", "edge_dst", "edge_type", "atom_ids", "flat"]
    kwonly = {k for k, p in inspect.signature(PT.__init__).parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert {"lr", "betas", "eps", "weight_decay", "max_grad_norm", "max_workspace_bytes"} <= kwonly
    for m in ("grad", "apply", "step", "state", "load_state", "set_lr", "weights", "workspace_bytes"):
        assert callable(getattr(PT, m))
    for mod, lead in (("ambient", ["self", "batch0", "batch1"]), ("latent", ["self", "batch"])):
        T = import_module(f"thermodynamic-interpolation_amd.thermo.{mod}").Trainer
        assert sig(T.__init__) == ["self", "b", "loss_fn", "lr", "weight_decay", "max_grad_norm", "betas", "eps", "max_workspace_bytes"]
        d = inspect.signature(T.__init__).parameters
        assert d["weight_decay"].default == 0.0 and d["max_grad_norm"].default == 1.0
        for m in ("step", "loss"):
            assert sig(getattr(T, m)) == lead + ["t", "z", "seed", "draw", "traj_offset", "center"]
        for m in ("set_lr", "sync", "state_dict", "load_state_dict"):
            assert callable(getattr(T, m))


def test_trainer_refuses_masked_and_mixed_batches_before_the_device():
    from importlib import import_module
    from types import SimpleNamespace
    ti = pkg()
    amb = import_module("thermodynamic-interpolation_amd.thermo.ambient")
    b = amb.cPaiNN(n_features=32, score_layers=1)
    tr = amb.Trainer(b, amb.losses.StandardVelocityLoss(amb.interpolants.LinearInterpolant(a=0.9, gamma="brownian")), lr=1e-3)
    A, B = 3, 2
    src, dst, et = ti.synthetic.fully_connected_template(A)
    ei = ti.synthetic.batch_edge_index(src, dst, A, B)
    mk = lambda ei, et, atoms: SimpleNamespace(x=np.zeros((B * A, 3), np.float32), T=np.full(B * A, 300.0, np.float32), atoms=atoms,
                                                edge_index=ei, edge_type=et, batch=np.repeat(np.arange(B), A))
    atoms = np.tile(np.arange(A), B)
    masked = mk(ei[:, :-1], np.tile(et, B)[:-1], atoms)                       # the second molecule lacks an edge
    mixed = mk(ei, np.tile(et, B), np.concatenate([np.arange(A), np.arange(A) + 1]))
    for bad in (masked, mixed):
        with pytest.raises(NotImplementedError):
            tr.step(bad, bad)
