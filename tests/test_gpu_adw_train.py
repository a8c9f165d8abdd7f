"""The adw trainer on the GPU (ti_adw_train_*): gradients against the fp64 restatement over the shape matrix and against the reference
fixtures, bit-for-bit repetition, clip + Adam against the restatement, the composition of the calls, the NaN skip, a short training
run, the driver, and the refusals that need a device.

Bars.  Gradients: per parameter tensor, rel-L2 against the fp64 restatement <= max(1e-5, 3 x the plain float32 model's distance for
the same case), the convention of the adw kernels.  Loss rows: the bound of tests/test_gpu_vloss.py from the drift
bar 1e-5 by Cauchy-Schwarz plus the reduction's 2 n_terms 2^-53 sum|terms|.  Optimiser: 16 k 2^-53 (|p| + lr) after k steps."""
import os
import types

import numpy as np
import pytest

import adw_train_numpy as an
import vloss_numpy as vn
from conftest import GOLDEN, ROOT, load_golden, pkg

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
MATRIX = [(32, 1, 1), (32, 3, 2), (64, 1, 3), (64, 5, 1), (128, 2, 4), (256, 1, 5), (256, 16, 2)]
MATRIX_B = (1, 17, 209, 1100)
KINDS = ["standard", "one_sided"]
A = 0.9


def _sh(v, d):
    """[B, d] -> the engine's shape ([B] at d = 1)"""
    return None if v is None else (np.ascontiguousarray(v[:, 0]) if d == 1 else v)


def _trainer(sd, H, L, d, **kw):
    return pkg().engine.AdwTrainer(H, L, an.flat(sd, H, L, d), dim=d, **kw)


def _drift_engine(sd, H, L, d):
    return pkg().engine.AdwEngine(H, L, an.flat(sd, H, L, d), dim=d)


def _loss_bound(x0, x1, t, z, ref_b, kind):
    """test_gpu_vloss._ref_bound for [B, d] rows"""
    B = x0.shape[0]
    f = lambda v: np.asarray(v, np.float64).reshape(B, -1)
    dd = f(x1) - f(x0)
    gz = 0.0 if kind == "one_sided" else vn.gamma_dot("brownian", A, np.asarray(t, np.float64))[:, None] * f(z)
    nrm = lambda v: np.linalg.norm(v, axis=1)
    bound = (nrm(ref_b[0]) + nrm(dd + gz)) * 1e-5 * np.linalg.norm(ref_b[0])
    if kind == "standard":
        bound = bound + (nrm(ref_b[1]) + nrm(dd - gz)) * 1e-5 * np.linalg.norm(ref_b[1])
    _, mag, n_terms = vn.loss(x0, x1, t, z, ref_b[0], ref_b[1] if kind == "standard" else None, kind=kind, gamma_kind="brownian", a=A)
    return bound + 2 * n_terms * U * mag


def _check_gradients(tag, r, H, L, d, sd, x0, x1, b0, b1, t, z, kind):
    ref = an.loss_and_grad(sd, x0, x1, b0, b1, t, z, kind=kind, a=A)
    m32 = an.per_tensor_rel_l2(an.loss_and_grad(sd, x0, x1, b0, b1, t, z, kind=kind, a=A, dtype=np.float32)["grads"], ref["grads"])
    err = an.per_tensor_rel_l2(an.unflat(r["grad"], H, L, d), ref["grads"])
    worst = max(err, key=lambda k: err[k] / max(1e-5, 3 * m32[k]))
    print(f"{tag}: worst {worst} {err[worst]:.2e} (float32 model {m32[worst]:.2e}); largest {max(err.values()):.2e}")
    for k in err:
        assert err[k] <= max(1e-5, 3 * m32[k]), (tag, k, err[k], m32[k])
    bound = _loss_bound(x0, x1, t, z, ref["b"], kind)
    assert (np.abs(r["loss"] - ref["loss"]) <= bound).all(), tag
    assert abs(r["mean"] - ref["mean"]) <= bound.sum() / len(t), tag
    # | |g| - |ref| | <= |g - ref|, and the tensors' bars bound that
    gf = an.flat(ref["grads"], H, L, d)
    bar = np.sqrt(sum((max(1e-5, 3 * m32[k]) * np.linalg.norm(ref["grads"][k])) ** 2 for k in err))
    assert abs(r["gnorm"] - np.sqrt(np.sum(gf * gf))) <= bar, tag
    return bound


# ------------------------------------------------------------------------------------------------ 1. gradients
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H, d, L", MATRIX)
def test_gradient_matrix(H, d, L, kind):
    """Every B of the matrix with per-row beta and with one shared beta pair, each with a given (t, z) and with a drawn one -- read back
    through ti_adw_vloss_interp of a drift handle, which draws them by the same kernels.  The loss rows and their mean also against
    ti_adw_vloss on that f32 drift handle, within the same bound as against fp64."""
    for B in MATRIX_B:
        for rows in (True, False):
            for drawn in (False, True):
                sd, x0, x1, b0, b1, t, z = an.case(H, d, L, B, per_row_beta=rows)
                zz = z if kind == "standard" else None
                tr, eng = _trainer(sd, H, L, d), _drift_engine(sd, H, L, d)
                if drawn:
                    kw = dict(seed=11, draw=3, traj_offset=5)
                    res = eng.interpolate(_sh(x0, d), _sh(x1, d), kind=kind, a=A, **kw)
                    t = res["t"]
                    zz = res["z"].reshape(B, d) if kind == "standard" else None
                else:
                    kw = dict(t=t, z=_sh(zz, d))
                r = tr.grad(_sh(x0, d), _sh(x1, d), b0, b1, kind=kind, a=A, **kw)
                tag = f"H{H} d{d} L{L} B{B} {kind} {'per-row' if rows else 'shared'} beta, {'drawn' if drawn else 'given'} (t, z)"
                bound = _check_gradients(tag, r, H, L, d, sd, x0, x1, b0, b1, t, zz, kind)
                v = eng.velocity_loss(_sh(x0, d), _sh(x1, d), b0, b1, kind=kind, a=A, **kw)
                assert abs(r["mean"] - v["mean"]) <= bound.sum() / B, tag
                assert (np.abs(r["loss"] - v["loss"]) <= bound).all(), tag
                tr.close(); eng.close()


def _fixture_sd(g):
    ti = pkg()
    H, L, d = int(g["hidden"]), int(g["num_layers"]), int(g["dim"])
    if d == 1:
        return ti.synthetic.adw_state_dict(H, L, int(g["seed"])), H, L, d
    return ti.synthetic.make_state_dict(ti.weights.adw_param_spec(H, L, d, d), seed=int(g["seed"]), dtype=np.float64), H, L, d


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["adw_train_h64", "adw_train_d3"])
def test_reference_fixture_gradients(name, kind):
    """The reference's autograd gradients (float64) directly, at its recorded (t, z)"""
    g = load_golden(name)
    sd, H, L, d = _fixture_sd(g)
    B = int(g["B"])
    x0, x1 = g["x0"].reshape(B, d), g["x1"].reshape(B, d)
    t, z = g[f"{kind}::t"], (g[f"{kind}::z"].reshape(B, d) if kind == "standard" else None)
    tr = _trainer(sd, H, L, d)
    r = tr.grad(_sh(x0, d), _sh(x1, d), g["beta0"], g["beta1"], kind=kind, a=float(g["a"]), t=t, z=_sh(z, d))
    ref = {k: g[f"{kind}::grad::{k}"] for k in sd}
    m32 = an.per_tensor_rel_l2(an.loss_and_grad(sd, x0, x1, g["beta0"], g["beta1"], t, z, kind=kind, a=float(g["a"]), dtype=np.float32)["grads"], ref)
    err = an.per_tensor_rel_l2(an.unflat(r["grad"], H, L, d), ref)
    print(name, kind, {k: f"{v:.1e}" for k, v in err.items()})
    for k in err:
        assert err[k] <= max(1e-5, 3 * m32[k]), (k, err[k], m32[k])
    assert abs(r["mean"] - float(g[f"{kind}::loss"])) <= 1e-5 * max(1.0, abs(float(g[f"{kind}::loss"])))


# ------------------------------------------------------------------------------------------------ 2. bits
def test_gradient_repeats_bit_for_bit_and_the_row_order_is_part_of_it():
    torch = pytest.importorskip("torch")
    g = load_golden("adw_train_h64")
    sd, H, L, d = _fixture_sd(g)
    B = int(g["B"])
    x0, x1, b0, b1, t, z = g["x0"][:, 0], g["x1"][:, 0], g["beta0"], g["beta1"], g["standard::t"], g["standard::z"][:, 0]
    tr = _trainer(sd, H, L, d)
    kw = dict(kind="standard", a=float(g["a"]))
    r1 = tr.grad(x0, x1, b0, b1, t=t, z=z, **kw)
    r2 = tr.grad(x0, x1, b0, b1, t=t, z=z, **kw)
    same = lambda a, b: all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("loss", "grad")) and a["mean"] == b["mean"] and a["gnorm"] == b["gnorm"]
    assert same(r1, r2)
    # device pointers
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    r3 = tr.grad(dev(x0), dev(x1), dev(b0), dev(b1), t=dev(t), z=dev(z), **kw)
    r3["loss"] = r3["loss"].cpu().numpy()
    assert same(r1, r3)
    # after an unrelated call with a larger B
    sdb, xa, xb, ba, bb, tb, zb = an.case(H, d, L, 700)
    tr.grad(xa[:, 0], xb[:, 0], ba, bb, t=tb, z=zb[:, 0], **kw)
    assert same(r1, tr.grad(x0, x1, b0, b1, t=t, z=z, **kw))
    # 64 sentinel rows behind the device output survive
    loss = torch.full((B + 64,), -7.0, dtype=torch.float64, device="cuda")
    ti = pkg()
    import ctypes as C
    desc = tr._desc("standard", "brownian", float(g["a"]), t, "uniform", 0, 0, 0)
    grad = np.full(tr.n_weights + 64, -7.0)
    arrs = [dev(v) for v in (x0, x1, b0, b1, t, z)]
    mean, gn = C.c_double(0), C.c_double(0)
    ti._lib.check(ti._lib.lib().ti_adw_train_grad(tr.h, C.byref(desc), *[C.c_void_p(a.data_ptr()) for a in arrs], B, C.c_void_p(loss.data_ptr()),
                                                  C.byref(mean), grad.ctypes.data_as(C.POINTER(C.c_double)), C.byref(gn), ti._lib.MEM_DEVICE))
    torch.cuda.synchronize()
    assert (loss[B:].cpu().numpy() == -7.0).all() and (grad[tr.n_weights:] == -7.0).all()
    assert np.array_equal(loss[:B].cpu().numpy(), r1["loss"]) and np.array_equal(grad[:tr.n_weights], r1["grad"])
    # the batch in another row order: the same gradient to round-off, not the same bits
    p = np.random.RandomState(0).permutation(B)
    r4 = tr.grad(x0[p], x1[p], b0[p], b1[p], t=t[p], z=z[p], **kw)
    assert np.array_equal(r4["loss"], r1["loss"][p])
    assert not np.array_equal(r4["grad"], r1["grad"]) and an.rel_l2(r4["grad"], r1["grad"]) <= 1e-5


# ------------------------------------------------------------------------------------------------ 3. apply
@pytest.mark.parametrize("wd", [0.0, 1e-5])
@pytest.mark.parametrize("max_norm, scale", [(1.0, 50.0), (1.0, 1e-3), (0.0, 50.0)], ids=["clip-active", "clip-inactive", "clip-off"])
def test_apply_against_the_restatement(max_norm, scale, wd):
    g = load_golden("adw_train_h64")
    sd, H, L, d = _fixture_sd(g)
    w = an.flat(sd, H, L, d)
    kw = dict(lr=1e-3, weight_decay=wd, max_grad_norm=max_norm)
    tr, ref = _trainer(sd, H, L, d, **kw), an.Adam(w, **kw)
    rs = np.random.RandomState(4)
    grads = [an.flat({k: g[f"standard::grad::{k}"] for k in sd}, H, L, d) * scale] + [rs.standard_normal(w.size) * scale for _ in range(4)]
    for k, gr in enumerate(grads):
        assert tr.apply(gr) is False and ref.step(gr) is False
        s = tr.state()
        assert s["n_applied"] == k + 1 and s["n_skipped"] == 0
        assert (np.abs(s["w"] - ref.w) <= an.adam_bound(ref.w, 1e-3, k + 1)).all()
        assert np.abs(s["m"] - ref.m).max() <= 16 * (k + 1) * U * np.abs(ref.m).max()
        assert np.abs(s["v"] - ref.v).max() <= 16 * (k + 1) * U * np.abs(ref.v).max()
    assert np.array_equal(tr.weights(), s["w"])
    # a NaN entry: skipped, and the state is the previous one bit for bit
    bad = grads[1].copy()
    bad[123] = np.nan
    assert tr.apply(bad) is True
    s2 = tr.state()
    assert s2["n_applied"] == 5 and s2["n_skipped"] == 1 and all(np.array_equal(s[k], s2[k]) for k in "wmv")
    bad[123] = np.inf
    assert tr.apply(bad) is True and tr.state()["n_skipped"] == 2


# ------------------------------------------------------------------------------------------------ 4. composition
def _same_state(a, b):
    sa, sb = a.state(), b.state()
    return all(np.array_equal(sa[k], sb[k]) for k in "wmv") and sa["n_applied"] == sb["n_applied"]


def _sets(n=600, seed=9):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(n).astype(np.float32), (1.5 * rs.standard_normal(n)).astype(np.float32),
            rs.choice([0.5, 1.0], n).astype(np.float32), rs.choice([1.25, 1.5], n).astype(np.float32))


def test_steps_compose_bit_for_bit():
    H, L, d, B = 64, 3, 1, 48
    sd = pkg().synthetic.adw_state_dict(H, L, 3)
    kw = dict(lr=1e-3, weight_decay=1e-5)
    X0, X1, B0, B1 = _sets()
    lk = dict(kind="standard", a=A, seed=5)
    # one step == grad then apply
    ta, tb = _trainer(sd, H, L, d, **kw), _trainer(sd, H, L, d, **kw)
    la, _ = ta.step(X0[:B], X1[:B], B0[:B], B1[:B], draw=2, **lk)
    r = tb.grad(X0[:B], X1[:B], B0[:B], B1[:B], draw=2, **lk)
    assert tb.apply(r["grad"]) is False and _same_state(ta, tb) and la == r["mean"]
    # six steps by index == six single steps on the gathered rows with draw = 0 .. 5
    rs = np.random.RandomState(1)
    i0, i1 = rs.randint(0, X0.size, (6, B)), rs.randint(0, X1.size, (6, B))
    tc, td = _trainer(sd, H, L, d, **kw), _trainer(sd, H, L, d, **kw)
    lc, skipped = tc.steps(X0, X1, B0, B1, i0, i1, **lk)
    ld = [td.step(X0[i0[k]], X1[i1[k]], B0[i0[k]], B1[i1[k]], draw=k, **lk)[0] for k in range(6)]
    assert skipped == 0 and np.array_equal(lc, np.asarray(ld)) and _same_state(tc, td) and tc.state()["n_applied"] == 6
    # indices in device memory give the same bits
    torch = pytest.importorskip("torch")
    te = _trainer(sd, H, L, d, **kw)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    le, _ = te.steps(dev(X0), dev(X1), dev(B0), dev(B1), dev(i0.astype(np.int64)), dev(i1.astype(np.int64)), **lk)
    assert np.array_equal(le, lc) and _same_state(te, tc)
    # get_state -> new trainer -> set_state -> continuing == uninterrupted
    tf, tg = _trainer(sd, H, L, d, **kw), _trainer(sd, H, L, d, **kw)
    tf.steps(X0, X1, B0, B1, i0[:3], i1[:3], **lk)
    tg.load_state(**tf.state())
    tg.steps(X0, X1, B0, B1, i0[3:], i1[3:], draw=3, **lk)
    assert _same_state(tg, tc)
    # an index out of range in device memory is refused before anything runs
    bad = i0.astype(np.int64).copy()
    bad[4, 7] = X0.size
    before = te.state()
    with pytest.raises(pkg()._lib.TiError, match=r"idx0\[199\]"):
        te.steps(dev(X0), dev(X1), dev(B0), dev(B1), dev(bad), dev(i1.astype(np.int64)), **lk)
    assert all(np.array_equal(before[k], te.state()[k]) for k in "wmv")


# ------------------------------------------------------------------------------------------------ 5. NaN skip inside a run
def test_nan_skip_inside_a_run():
    H, L, d, B = 64, 3, 1, 48
    sd = pkg().synthetic.adw_state_dict(H, L, 3)
    X0, X1, B0, B1 = _sets()
    X1 = np.concatenate([X1, np.asarray([np.inf], np.float32)])
    B1 = np.concatenate([B1, B1[:1]])
    rs = np.random.RandomState(2)
    i0, i1 = rs.randint(0, X0.size, (6, B)), rs.randint(0, X0.size, (6, B))
    i1[2, 17] = X1.size - 1                                   # the third minibatch holds the inf
    lk = dict(kind="standard", a=A, seed=5)
    ta, tb = _trainer(sd, H, L, d), _trainer(sd, H, L, d)
    la, skipped = ta.steps(X0, X1, B0, B1, i0, i1, **lk)
    assert skipped == 1 and np.isnan(la[2]) and np.isfinite(np.delete(la, 2)).all()
    s = ta.state()
    assert s["n_applied"] == 5 and s["n_skipped"] == 1
    lb = [tb.step(X0[i0[k]], X1[i1[k]], B0[i0[k]], B1[i1[k]], draw=k, **lk)[0] for k in (0, 1, 3, 4, 5)]   # a skipped step consumes its draw
    assert np.array_equal(np.delete(la, 2), np.asarray(lb)) and _same_state(ta, tb)


# ------------------------------------------------------------------------------------------------ 6. it trains
def test_it_trains():
    """1 500 steps at batch 512, lr 1e-3, from the reference-initialised weights (adw_ctor_h64) on Boltzmann pairs beta 1.0 -> 1.25 (the
    seeds of tests/golden/train_adw.py); the exported weights scored by ti_adw_vloss on the held-out 4 096 pairs of vloss_adw_trained.npz
    at its (seed, draw).  Condition: below the fixture's untrained mean by more than 5 of its standard errors."""
    ti = pkg()
    g, ref = load_golden("adw_ctor_h64"), load_golden("vloss_adw_trained")
    sd = {k[4:]: v for k, v in g.items() if k.startswith("sd::")}
    H, L = int(g["hidden"]), int(g["num_layers"])
    b = ti.thermo.adw.FCNetMultiBeta(1, 1, H, L).load_state_dict(sd)
    loss_fn = ti.thermo.losses.StandardVelocityLoss(ti.thermo.interpolants.LinearInterpolant(float(ref["a"])))
    N = 100_000
    x0, x1 = ti.synthetic.adw_boltzmann(N, float(ref["beta0"]), seed=1), ti.synthetic.adw_boltzmann(N, float(ref["beta1"]), seed=2)
    trainer = ti.thermo.adw.Trainer(b, loss_fn, 1e-3, weight_decay=1e-5)
    losses, skipped = trainer.fit(x0, x1, float(ref["beta0"]), float(ref["beta1"]), 512, 1500, 0)
    trainer.sync()
    n = int(ref["n"])
    h0 = ti.synthetic.adw_boltzmann(n, float(ref["beta0"]), seed=int(ref["seed_x0"])).astype(np.float32)
    h1 = ti.synthetic.adw_boltzmann(n, float(ref["beta1"]), seed=int(ref["seed_x1"])).astype(np.float32)
    got = loss_fn(b, h0, h1, np.full(n, float(ref["beta0"]), np.float32), np.full(n, float(ref["beta1"]), np.float32), seed=int(ref["seed"]), draw=int(ref["draw"]))
    text = (f"adw trainer, H = {H}, L = {L}: 1500 steps at batch 512, lr 1e-3, weight_decay 1e-5 from adw_ctor_h64\n"
            f"held-out velocity loss (4096 pairs, seed {int(ref['seed'])}, draw {int(ref['draw'])}): {got:.6f}\n"
            f"fixture: untrained {float(ref['untrained_mean']):.6f} +- {float(ref['untrained_sem']):.6f}, "
            f"trained by the reference (6000 steps, decaying lr) {float(ref['trained_mean']):.6f} +- {float(ref['trained_sem']):.6f}\n"
            f"training loss: first 50 steps {losses[:50].mean():.5f}, last 50 steps {losses[-50:].mean():.5f}; skipped {skipped}\n")
    print(text)
    with open(os.path.join(ROOT, "profiles", "adw_train_bench.txt"), "w") as f:
        f.write(text)
    assert skipped == 0
    assert got < float(ref["untrained_mean"]) - 5 * float(ref["untrained_sem"])


# ------------------------------------------------------------------------------------------------ 7. driver
def test_driver_writes_checkpoints_that_score_and_resume(tmp_path):
    ti = pkg()
    n = 4096
    base = (ti.synthetic.adw_boltzmann(n, 1.0, seed=1).astype(np.float32), 1.0)
    target = (ti.synthetic.adw_boltzmann(n, 1.25, seed=2).astype(np.float32), 1.25)
    cfg = lambda name, epochs: types.SimpleNamespace(hidden_size=64, num_layers=3, lr=1e-3, wd=1e-5, batch_size=128, epochs=epochs, a=0.9, seed=0,
                                                     model_save_path=str(tmp_path), model_save_name=name)
    log = ti.drivers.train_adw(cfg("full", 2), base, target)
    out = tmp_path / "full"
    assert sorted(p.name for p in out.iterdir()) == ["epoch_0.npz", "epoch_1.npz", "log.npz", "train_state.npz"]
    with np.load(out / "log.npz") as f:
        assert sorted(f.files) == ["lr", "skipped", "train_loss", "val_loss"] and all(f[k].shape == (2,) for k in f.files)
        assert np.array_equal(f["val_loss"], log["val_loss"]) and (f["skipped"] == 0).all() and (f["lr"] == 1e-3).all()
    with np.load(out / "epoch_1.npz") as f:
        assert f["net.0.weight"].dtype == np.float64 and f["net.0.weight"].shape == (64, 3) and len(f.files) == 14
    # score_checkpoints reads them: epoch 1 is not worse than epoch 0 beyond the standard error
    m = 1024
    h0, h1 = ti.synthetic.adw_boltzmann(m, 1.0, seed=11).astype(np.float32), ti.synthetic.adw_boltzmann(m, 1.25, seed=12).astype(np.float32)
    sc = types.SimpleNamespace(gamma="brownian", t_distr="uniform", interpolant_a=0.9, seed=3, data_save_path=str(tmp_path), data_save_name="score")
    b = ti.thermo.adw.FCNetMultiBeta(1, 1, 64, 3)
    res = ti.drivers.score_checkpoints(sc, b, [(h0, h1, np.full(m, 1.0, np.float32), np.full(m, 1.25, np.float32))],
                                       [str(out / "epoch_0.npz"), str(out / "epoch_1.npz")])
    print("driver: val loss per epoch", log["val_loss"], "held-out score", res["mean"], "+-", res["sem"])
    assert res["mean"][1] <= res["mean"][0] + res["sem"][0]
    # resume after epoch 0 == the uninterrupted run, bit for bit
    ti.drivers.train_adw(cfg("cut", 1), base, target)
    ti.drivers.train_adw(cfg("cut", 2), base, target, resume=True)
    for name in ("epoch_0.npz", "epoch_1.npz", "log.npz"):
        with np.load(out / name) as fa, np.load(tmp_path / "cut" / name) as fb:
            assert sorted(fa.files) == sorted(fb.files) and all(np.array_equal(fa[k], fb[k]) for k in fa.files), name


# ------------------------------------------------------------------------------------------------ 8. refusals on the device
def test_refusals_on_the_device():
    import ctypes as C
    ti = pkg()
    L_ = ti._lib.lib()
    H, L, d = 32, 2, 1
    sd = ti.synthetic.adw_state_dict(H, L, 0)
    with pytest.raises(ti._lib.TiError, match="TI_PREC_F32 only"):
        ti.engine.AdwTrainer(H, L, an.flat(sd, H, L, d), precision="f16x2")
    tr, eng = _trainer(sd, H, L, d), _drift_engine(sd, H, L, d)
    x = np.zeros(4, np.float32)
    p = x.ctypes.data_as(C.c_void_p)
    # a trainer handle into the drift and the velocity loss
    assert L_.ti_adw_drift(tr.h, p, C.c_float(0.5), p, p, 4, p, 0) == ti._lib.TI_E_ARG and "not an adw handle" in ti._lib.last_error()
    desc = tr._desc("standard", "brownian", A, None, "uniform", 0, 0, 0)
    loss = np.zeros(4)
    assert L_.ti_adw_vloss(tr.h, C.byref(desc), p, p, p, p, None, None, 4, loss.ctypes.data_as(C.c_void_p), None, None, None, None, None, None, 0) == ti._lib.TI_E_ARG
    assert "not an adw handle" in ti._lib.last_error()
    # a drift handle into the trainer calls
    assert L_.ti_adw_train_grad(eng.h, C.byref(desc), p, p, p, p, None, None, 4, None, None, None, None, 0) == ti._lib.TI_E_ARG
    assert "not an adw trainer handle" in ti._lib.last_error()
    g = np.zeros(tr.n_weights)
    assert L_.ti_adw_train_apply(eng.h, g.ctypes.data_as(C.POINTER(C.c_double)), None) == ti._lib.TI_E_ARG
    assert L_.ti_adw_train_get_state(eng.h, None, None, None, None, None) == ti._lib.TI_E_ARG
    # the shared calls that size or read a drift handle's state refuse a trainer too
    assert L_.ti_reserve(tr.h, 8) == ti._lib.TI_E_ARG and "trainer" in ti._lib.last_error()
    desc_cv = np.asarray([ti._lib.OBS_KINDS["coord"], 0, 0, 0, 0], np.int32)
    assert L_.ti_obs_cv(tr.h, ti._lib.iptr(desc_cv), 1, None, None, p, 4, p, 0) == ti._lib.TI_E_ARG and "trainer" in ti._lib.last_error()
    assert L_.ti_reserve(eng.h, 8) == ti._lib.TI_OK
    # both still work
    assert np.isfinite(tr.step(x, x + 1, x + 1, x + 1.25, a=A)[0]) and np.isfinite(eng.drift(x, 0.5, x + 1, x + 1.25)).all()
