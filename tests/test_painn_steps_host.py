"""Whole epochs of the molecule trainer without a GPU: the new symbols, every refusal of ti_painn_train_steps, ti_painn_train_noise and
ti_painn_train_best that is raised before the device in the order include/ti_hip.h states, the numpy restatement of the aligned base
samples against scipy and against the stored fixture, and the drivers against a stub trainer."""
import ctypes as C
import inspect
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import painn_noise_numpy as pn
from conftest import load_golden, pkg


@pytest.fixture(scope="module")
def lib():
    ti = pkg()
    ti.build.build()
    return ti._lib.lib()


def test_sources_and_symbols_are_listed(lib):
    ti = pkg()
    assert "painn_steps_kernels.hip" in ti.build.SOURCES and "painn_noise_kernels.hip" in ti.build.SOURCES and "painn_steps.hpp" in ti.build.HEADERS
    header = open(os.path.join(os.path.dirname(ti.__file__), "..", "include", "ti_hip.h")).read()
    for n in ("ti_painn_train_steps", "ti_painn_train_best", "ti_painn_train_noise"):
        assert n in ti._lib.ABI_SYMBOLS and hasattr(lib, n) and f"int {n}(ti_handle* h" in header
    assert "enum { TI_NOISE_GIVEN = 0, TI_NOISE_DRAWN = 1, TI_NOISE_ALIGNED = 2 };" in header
    assert ti._lib.PAINN_NOISES == {"given": 0, "drawn": 1, "aligned": 2}
    assert C.sizeof(ti._lib.PainnStepsDesc) == 24
    assert lib.ti_version() == 5


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_steps_refusals_come_in_the_stated_order(lib):
    """With a NULL handle, word by word as the header lists the checks; each case is also wrong in what comes later, so the earlier
    check is the one that answers.  (The workspace, the temperatures, the ambient and A < 3 refusals need a trainer:
    tests/test_gpu_painn_steps.py.)"""
    ti = pkg()
    E = ti._lib.TI_E_ARG
    D = lambda **kw: ti._lib.VlossDesc(**{**dict(kind=0, gamma=1, a=1.0, center=0, t_dist=1, seed=0, traj_offset=0, draw=0, n_tbins=0), **kw})
    S = lambda n=2, update=1, noise=0, best=0: ti._lib.PainnStepsDesc(n, update, noise, best)
    x = np.zeros(4 * 9, np.float32)
    idx = np.zeros(4, np.int64)
    xp, ip = x.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)
    bad_idx = np.asarray([0, 1, 7, 0], np.int64)
    bp = bad_idx.ctypes.data_as(C.c_void_p)

    def steps(desc=D(), sd=S(), x0=xp, n0=4, x1=xp, n1=4, i0=ip, i1=ip, B=2, mem=0):
        return lib.ti_painn_train_steps(None, C.byref(desc) if desc is not None else None, C.byref(sd) if sd is not None else None, x0, n0, None,
                                        x1, n1, None, i0, i1, B, None, None, mem)

    one = D(kind=1)
    cases = [("desc is NULL", dict(desc=None, sd=None)), ("loss kind", dict(desc=D(kind=5), sd=None)), ("B < 1", dict(B=0, sd=None)),
             ("unknown mem", dict(mem=9, sd=None)), ("GIVEN needs t", dict(desc=D(t_dist=0), sd=None)),
             ("steps desc is NULL", dict(sd=None, i0=None)), ("n_steps must be", dict(sd=S(n=0, update=7))), ("n_steps must be", dict(sd=S(n=1 << 31, update=7))),
             ("unknown update", dict(sd=S(update=7, noise=9))), ("unknown noise", dict(sd=S(noise=9, best=5))), ("unknown track_best", dict(sd=S(best=5, noise=1))),
             ("must be ONE_SIDED", dict(sd=S(noise=1, update=0, best=1))), ("x0 must be NULL", dict(desc=one, sd=S(noise=2, update=0, best=1))),
             ("track_best needs update", dict(sd=S(update=0, best=1), i0=None)),
             ("both be given or both be NULL", dict(i0=None, n1=0)), ("without indices n_steps must be 1", dict(i0=None, i1=None, n1=0)),
             ("do not cover", dict(n1=0, x1=None)), ("do not cover", dict(n0=0, x1=None)), ("do not cover", dict(sd=S(n=1), i0=None, i1=None, n0=1, x1=None)),
             ("overflows the draw index", dict(desc=D(draw=(1 << 31) - 1), x1=None)),
             ("NULL buffer", dict(x1=None, i0=bp)), ("NULL buffer", dict(x0=None, i0=bp)),
             ("idx0[2] is outside", dict(i0=bp)), ("idx1[2] is outside", dict(i1=bp)),
             ("not a painn trainer handle", dict()),
             # drawn noise: no set 0, so neither n0 nor the values of idx0 are looked at
             ("not a painn trainer handle", dict(desc=one, sd=S(noise=1), x0=None, n0=0, i0=bp)),
             ("idx1[2] is outside", dict(desc=one, sd=S(noise=2), x0=None, n0=0, i1=bp))]
    for word, kw in cases:
        assert steps(**kw) == E and word in lib.ti_last_error().decode(), (word, kw, lib.ti_last_error().decode())
    assert steps(mem=1) == E and "not a painn trainer handle" in lib.ti_last_error().decode()      # device indices are not read without a trainer


def test_noise_and_best_refusals(lib):
    ti = pkg()
    E = ti._lib.TI_E_ARG
    x = np.zeros(18, np.float32)
    xp = x.ctypes.data_as(C.c_void_p)

    def noise(kind=2, B=2, draw=0, mem=0, x1=xp, out=xp):
        return lib.ti_painn_train_noise(None, 0, 0, draw, x1, B, kind, out, None, mem)

    for word, kw in (("TI_NOISE_DRAWN or TI_NOISE_ALIGNED", dict(kind=0, B=0)), ("TI_NOISE_DRAWN or TI_NOISE_ALIGNED", dict(kind=3, B=0)),
                     ("B < 1", dict(B=0, draw=-1)), ("draw < 0", dict(draw=-1, mem=9)), ("unknown mem", dict(mem=9, out=None)),
                     ("NULL buffer", dict(out=None, x1=None)), ("needs x1", dict(x1=None)), ("not a painn trainer handle", dict()),
                     ("not a painn trainer handle", dict(kind=1, x1=None))):
        assert noise(**kw) == E and word in lib.ti_last_error().decode(), (word, lib.ti_last_error().decode())
    assert lib.ti_painn_train_best(None, None, None, None, 0) == E and "not a painn trainer handle" in lib.ti_last_error().decode()


# ------------------------------------------------------------------------------------------------ the rotation restated
GROUPS = ("a3", "a9")


def test_fixture_holds_the_stated_molecules():
    z = load_golden("painn_noise_align")
    assert z["x1_a3"].shape == (4, 3, 3) and z["x1_a9"].shape == (12, 9, 3) and z["x1_a3"].dtype == np.float32
    for g in GROUPS:
        assert z[f"x0_{g}"].dtype == z[f"rot_{g}"].dtype == z[f"aligned_{g}"].dtype == np.float64
        assert (z[f"gap_{g}"] >= 1e-3).all()
        for b in range(z[f"x1_{g}"].shape[0]):
            assert pn.horn_gap(z[f"x1_{g}"][b].astype(np.float64), z[f"x0_{g}"][b]) == pytest.approx(z[f"gap_{g}"][b], rel=1e-9)
    for b in range(4):                                         # three centred points are coplanar: the correlation matrix has rank 2
        s = np.linalg.svd(z["x1_a3"][b].astype(np.float64).T @ z["x0_a3"][b], compute_uv=False)
        assert s[2] <= 1e-6 * s[0] < s[1]
    assert np.array_equal(z["x1_a9"][0], z["x0_a9"][0].astype(np.float32))                              # the identity
    assert np.array_equal(z["x1_a9"][1], (z["x0_a9"][1] * np.array([-1.0, 1.0, 1.0])).astype(np.float32))      # the mirror image
    U, _, Vt = np.linalg.svd(z["x1_a9"][1].astype(np.float64).T @ z["x0_a9"][1])
    assert np.linalg.det(U @ Vt) < 0.0


@pytest.mark.parametrize("g", GROUPS)
def test_restatement_against_the_fixture(g):
    """The draws are the oracle's, the centring is exact, Kabsch by numpy.linalg.svd agrees with scipy's stored R within 1e-12"""
    z = load_golden("painn_noise_align")
    x1 = z[f"x1_{g}"]
    got, R, xc = pn.noise(int(z["seed"]), int(z[f"traj_offset_{g}"]), int(z["draw"]), x1, True)
    assert np.array_equal(xc, z[f"x0_{g}"])
    assert np.abs(R - z[f"rot_{g}"]).max() <= 1e-12 and np.abs(np.linalg.det(R) - 1.0).max() <= 1e-12
    assert np.abs(np.einsum("bij,baj->bai", R, xc) - z[f"aligned_{g}"]).max() <= 1e-11
    want = z[f"aligned_{g}"]
    assert (np.abs(got.astype(np.float64) - want.astype(np.float32)) <= 2.0 ** -23 * np.abs(want).max(axis=(1, 2), keepdims=True)).all()
    # R minimises: every small rotation away from it is worse
    rs = np.random.RandomState(0)
    for b in range(x1.shape[0]):
        cost = lambda Rm: float(((x1[b].astype(np.float64) - xc[b] @ Rm.T) ** 2).sum())
        for _ in range(4):
            w = 1e-3 * rs.standard_normal(3)
            Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            Q, _ = np.linalg.qr(np.eye(3) + Wx)
            Q = Q * np.sign(np.diag(Q @ np.eye(3)))            # a proper rotation near the identity
            assert cost(R[b]) <= cost(Q @ R[b]) + 1e-12


@pytest.mark.parametrize("g", GROUPS)
def test_restatement_against_scipy(g):
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    z = load_golden("painn_noise_align")
    for b in range(z[f"x1_{g}"].shape[0]):
        x1, x0 = z[f"x1_{g}"][b].astype(np.float64), z[f"x0_{g}"][b]
        assert np.abs(pn.kabsch(x1, x0) - Rotation.align_vectors(x1, x0)[0].as_matrix()).max() <= 1e-12


def test_centring_sums_in_atom_order():
    x = np.asarray([[[1e8, 1.0, -1.0], [1.0, 2.0 ** -20, 3.0], [-1e8, 5.0, 2.0 ** -24], [3.0, 1e-3, 0.25]]], np.float32)
    xc = pn.centre(x)
    s = np.zeros(3)
    for a in range(4):
        s = s + x[0, a].astype(np.float64)
    assert np.array_equal(xc[0], x[0].astype(np.float64) - s / 4.0)


# ------------------------------------------------------------------------------------------------ the drivers without a device
def _config(tmp, **kw):
    base = dict(n_features=32, score_layers=1, batch_size=5, n_epochs=2, learning_rate=1e-3, weight_decay=0.0, a=1.0, gamma="brownian", t_distr="uniform",
                seed=3, align=False, model_save_path=str(tmp), model_save_name="run")
    base.update(kw)
    return SimpleNamespace(**{k: v for k, v in base.items() if v is not ...})


def _sets(n0=17, n1=19, A=3):
    rs = np.random.RandomState(0)
    mk = lambda n: (rs.standard_normal((n, A, 3)).astype(np.float32), np.full(n, 300.0, np.float32))
    return mk(n0), mk(n1)


@pytest.mark.parametrize("which", ["ambient", "latent"])
def test_driver_config_checks_come_before_any_device_work(which, tmp_path, monkeypatch):
    ti = pkg()
    mod = import_module(f"thermodynamic-interpolation_amd.thermo.{which}")

    def boom(*a, **k):
        raise AssertionError("the trainer was built before the config was checked")
    monkeypatch.setattr(mod, "Trainer", boom)
    set0, set1 = _sets()
    run = (lambda cfg, s0=set0, s1=set1: ti.drivers.train_ambient(cfg, s0, s1, None)) if which == "ambient" else \
          (lambda cfg, s0=None, s1=set1: ti.drivers.train_latent(cfg, s1, None))
    bad = [("n_features", 48), ("n_features", 32.0), ("score_layers", 0), ("batch_size", 0), ("batch_size", True), ("n_epochs", 0), ("learning_rate", 0.0),
           ("learning_rate", float("nan")), ("weight_decay", -1.0), ("a", 0.0), ("gamma", "cubic"), ("t_distr", "normal"), ("seed", -1), ("align", "yes"),
           ("model_save_path", ""), ("model_save_name", None), ("n_features", ...), ("learning_rate", ...)]
    if which == "ambient":
        bad.append(("align", True))
    for key, v in bad:
        with pytest.raises(ValueError, match=f"config.{key}"):
            run(_config(tmp_path, **{key: v}))
    with pytest.raises(ValueError, match="no full training batch"):
        run(_config(tmp_path, batch_size=64))
    with pytest.raises(ValueError, match=r"\[n, A, 3\]"):
        run(_config(tmp_path), s1=(np.zeros((4, 9)), np.zeros(4)))
    with pytest.raises(ValueError, match="draw indices"):
        run(_config(tmp_path, n_epochs=1 << 29))
    assert not os.listdir(tmp_path)


class _StubTrainer:
    """Stands where thermo.ambient.Trainer / thermo.latent.Trainer stand in the drivers: records the calls, returns scripted losses"""
    calls = []

    def __init__(self, b, loss_fn, lr, weight_decay=0.0, max_grad_norm=1.0):
        self.b, self.loss_fn, self.lr, self.n, self.epoch = b, loss_fn, float(lr), 0, 0
        type(self).calls.append(("init", type(loss_fn).__name__, lr, weight_decay, max_grad_norm))

    def fit(self, *a, **kw):
        type(self).calls.append(("fit", a, kw))
        steps = a[-2]
        self.n += steps
        self.epoch += 1
        return np.full(steps, 2.0) + np.arange(steps), 0          # the same training loss in every epoch: a plateau

    def evaluate(self, *a, **kw):
        type(self).calls.append(("evaluate", a, kw))
        return np.full(a[-2], 1.5)

    def best_state_dict(self, reset=False):
        type(self).calls.append(("best", reset))
        return {k: v + 1 for k, v in self.b.state_dict().items()}, 2.0, 0

    def set_lr(self, lr):
        type(self).calls.append(("set_lr", lr))
        self.lr = float(lr)

    def sync(self):
        return self.b

    def state_dict(self):
        return dict(w=np.zeros(3), m=np.zeros(3), v=np.zeros(3), n_applied=self.n, n_skipped=0, lr=self.lr)

    def load_state_dict(self, st):
        type(self).calls.append(("load", int(st["n_applied"]), float(st["lr"])))
        self.n, self.lr = int(st["n_applied"]), float(st["lr"])
        return self


@pytest.mark.parametrize("which", ["ambient", "latent"])
def test_driver_bookkeeping_against_a_stub_trainer(which, tmp_path, monkeypatch):
    """The files written, what an epoch calls and with which draws, _Plateau driven by the training loss, and the resume."""
    ti = pkg()
    mod = import_module(f"thermodynamic-interpolation_amd.thermo.{which}")
    monkeypatch.setattr(mod, "Trainer", _StubTrainer)
    _StubTrainer.calls = []
    set0, set1 = _sets()
    latent = which == "latent"
    tpl = object()
    run = (lambda cfg, **k: ti.drivers.train_latent(cfg, set1, tpl, **k)) if latent else (lambda cfg, **k: ti.drivers.train_ambient(cfg, set0, set1, tpl, **k))
    steps = 19 // 5 if latent else 17 // 5
    log = run(_config(tmp_path, n_epochs=12, align=latent))
    out = os.path.join(str(tmp_path), "run")
    want = {"train_state.npz", "log.npz"} | {f"run_{e}_weights.npz" for e in range(12)} | {f"run_best{e}_weights.npz" for e in range(12)}
    assert set(os.listdir(out)) == want
    assert set(log) == {"train_loss", "last_train_loss", "best_loss", "lr", "skipped"} and all(v.shape == (12,) for v in log.values())
    assert np.allclose(log["train_loss"], 2.0 + (steps - 1) / 2.0) and (log["last_train_loss"] == 1.5).all() and (log["best_loss"] == 2.0).all()
    # ReduceLROnPlateau(0.5, 10) on the TRAINING loss: epoch 0 sets the best, epochs 1..11 are bad, the 11th halves the rate
    assert (log["lr"] == 1e-3).all() and ("set_lr", 5e-4) in _StubTrainer.calls
    calls = _StubTrainer.calls
    assert calls[0][:2] == ("init", "OneSidedVelocityLoss" if latent else "StandardVelocityLoss") and calls[0][4] == 1.0
    fits = [c for c in calls if c[0] == "fit"]
    evals = [c for c in calls if c[0] == "evaluate"]
    assert len(fits) == len(evals) == 12 and [c for c in calls if c[0] == "best"] == [("best", True)] * 12
    D0 = ti.drivers._TRAIN_DRAW0
    for e, (f, v) in enumerate(zip(fits, evals)):
        assert f[1][-3:] == (5, steps, [3, 2, e]) and v[1][-3:] == (5, steps, [3, 2, e])           # the same fresh permutation for both passes
        assert f[2]["draw"] == D0 + 2 * e * steps and v[2]["draw"] == D0 + (2 * e + 1) * steps and f[2]["noise_seed"] == v[2]["noise_seed"] == 3
        assert f[2]["template_batch"] is tpl and f[2]["track_best"] is True
        if latent:
            assert f[2]["noise"] == v[2]["noise"] == "aligned" and len(f[1]) == 5 and f[1][0] is not None and f[1][0].shape == (19, 3, 3)
        else:
            assert len(f[1]) == 7 and f[1][0].shape == (17, 3, 3) and f[1][2].shape == (19, 3, 3) and f[1][1].shape == (17,)
    with np.load(os.path.join(out, "run_best3_weights.npz")) as p, np.load(os.path.join(out, "run_3_weights.npz")) as q:
        assert set(p.files) == set(q.files) and all(np.array_equal(p[k], q[k] + 1) for k in p.files)
    with np.load(os.path.join(out, "train_state.npz")) as st:
        assert int(st["epochs_done"]) == 12 and float(st["sched_lr"]) == 5e-4 and st["log_train_loss"].shape == (12,) and int(st["n_applied"]) == 12 * steps
    # resume: two more epochs continue the counters, the scheduler and the log
    _StubTrainer.calls = []
    more = run(_config(tmp_path, n_epochs=14, align=latent), resume=True)
    assert ("load", 12 * steps, 5e-4) in _StubTrainer.calls and len([c for c in _StubTrainer.calls if c[0] == "fit"]) == 2
    assert more["lr"].shape == (14,) and (more["lr"][12:] == 5e-4).all() and np.array_equal(more["train_loss"][:12], log["train_loss"])
    assert [c[1][-1] for c in _StubTrainer.calls if c[0] == "fit"] == [[3, 2, 12], [3, 2, 13]]
    assert os.path.exists(os.path.join(out, "run_13_weights.npz"))


def test_python_surface():
    ti = pkg()
    sig = lambda f: list(inspect.signature(f).parameters)
    PT = ti.engine.PainnTrainer
    assert sig(PT.__init__)[:10] == ["self", "variant", "F", "L", "A", "edge_src", "edge_dst", "edge_type", "atom_ids", "flat"]
    assert sig(PT.steps)[:7] == ["self", "x0", "x1", "temp0", "temp1", "idx0", "idx1"] and {"update", "noise", "track_best", "draw"} <= set(sig(PT.steps))
    assert callable(PT.noise) and sig(PT.best) == ["self", "reset"]
    base = import_module("thermodynamic-interpolation_amd.thermo._molecule").MoleculeTrainerBase
    for m in ("fit", "evaluate", "best_state_dict"):
        assert callable(getattr(base, m))
    amb, lat = (import_module(f"thermodynamic-interpolation_amd.thermo.{m}").Trainer for m in ("ambient", "latent"))
    assert sig(amb.fit)[:8] == ["self", "x0", "temps0", "x1", "temps1", "batch_size", "n_steps", "seed"]
    assert sig(lat.fit)[:6] == ["self", "x1", "temps1", "batch_size", "n_steps", "seed"] and inspect.signature(lat.fit).parameters["noise"].default == "drawn"
    assert sig(ti.drivers.train_ambient) == ["config", "set0", "set1", "template", "resume"]
    assert sig(ti.drivers.train_latent) == ["config", "set1", "template", "resume"]
    with pytest.raises(ValueError, match="template_batch"):
        b = import_module("thermodynamic-interpolation_amd.thermo.ambient")
        tr = b.Trainer(b.cPaiNN(n_features=32, score_layers=1), b.losses.StandardVelocityLoss(b.interpolants.LinearInterpolant()), lr=1e-3)
        tr.fit(np.zeros((5, 3, 3), np.float32), np.zeros(5), np.zeros((5, 3, 3), np.float32), np.zeros(5), 5, 1, 0)
