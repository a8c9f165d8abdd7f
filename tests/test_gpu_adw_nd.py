"""FCNetMultiBeta(d, d, H, L) on the GPU: drift, exact divergence and every integrator against the reference fixtures
(tests/golden/make_golden_nd.py), the fp64 numpy restatement (adw_nd_numpy.py) and oracle/ode.py; the d = 1 handle of
ti_adw_create_nd against ti_adw_create bit for bit."""
import ctypes as C

import numpy as np
import pytest

from adw_nd_numpy import CASES, drift as np_drift, load_case
from conftest import load_golden, pkg, rel_l2
from oracle import ode

pytestmark = pytest.mark.gpu
F32 = np.float32


def _engine(g, sd, precision="f32"):
    ti = pkg()
    d, H, L = int(g["dim"]), int(g["hidden"]), int(g["num_layers"])
    flat = ti.weights.flatten_state_dict(sd, ti.weights.adw_param_spec(H, L, d, d), dtype=np.float64)
    return ti.engine.AdwEngine(H, L, flat, precision=precision, dim=d)


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return load_case(request.param)


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_drift_and_divergence_vs_reference(case, precision):
    g, sd = case
    eng = _engine(g, sd, precision)
    x = g["x"].astype(F32)
    for tag in ("", "_var"):
        b0, b1 = g["beta0" + tag].astype(F32), g["beta1" + tag].astype(F32)
        for key, t in [(str(i), float(t)) for i, t in enumerate(g["ts"])] + [("tv", g["tv"].astype(F32))]:
            b, div = eng.drift(x, t, b0, b1, return_div=True)
            assert b.shape == x.shape and div.shape == (x.shape[0],)
            assert rel_l2(b, g[f"drift{tag}_{key}"]) <= 1e-5, (tag, key)
            assert rel_l2(-div * 1e-2, g[f"negdiv{tag}_{key}"]) <= 1e-5, (tag, key)
            np.testing.assert_array_equal(eng.drift(x, t, b0, b1), b)      # drift-only kernel: same primal bits


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_euler_heun_paths_and_dlogp_vs_reference(case, precision):
    g, sd = case
    eng = _engine(g, sd, precision)
    x, b0, b1, grid = g["x"].astype(F32), g["beta0"].astype(F32), g["beta1"].astype(F32), g["traj_grid"].astype(F32)
    for scheme in ("euler", "heun"):
        path, nfe = eng.rollout(x, b0, b1, grid, scheme=scheme)
        assert path.shape == (len(grid),) + x.shape
        assert rel_l2(path, g[f"traj_{scheme}"]) <= 1e-5, scheme
        path2, dl, _ = eng.rollout(x, b0, b1, grid, scheme=scheme, return_dlogp=True)
        np.testing.assert_array_equal(path2, path)
        assert dl.shape == (len(grid), x.shape[0])
        assert rel_l2(dl[1:], g[f"dlogp_{scheme}"][1:]) <= 1e-5, scheme


def test_python_mirror_shapes(case):
    torch = pytest.importorskip("torch")
    g, sd = case
    ti = pkg()
    d, H, L = int(g["dim"]), int(g["hidden"]), int(g["num_layers"])
    net = ti.thermo.adw_nd.FCNetMultiBeta(d, d, H, L).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = torch.from_numpy(g["x"].astype(F32))
    b0, b1 = torch.from_numpy(g["beta0"].astype(F32))[:, None], torch.from_numpy(g["beta1"].astype(F32))[:, None]
    integ = ti.thermo.adw_nd.StandardIntegrator(b=net, method="euler", n_step=len(g["traj_grid"]), return_dlogp=True)
    path, dlogp = integ.rollout(x, b0, b1)
    assert tuple(path.shape) == (len(g["traj_grid"]), x.shape[0], d) and tuple(dlogp.shape) == (len(g["traj_grid"]), x.shape[0], 1)
    assert rel_l2(path.numpy(), g["traj_euler"]) <= 1e-5 and rel_l2(dlogp.numpy()[1:, :, 0], g["dlogp_euler"][1:]) <= 1e-5
    b, negdiv = ti.thermo.adw_nd.ODEWrapper(net, return_dlogp=True)(0.37, (x, None), None, b0, b1)
    assert rel_l2(b.numpy(), g["drift_1"]) <= 1e-5 and rel_l2(negdiv.numpy()[:, 0], g["negdiv_1"]) <= 1e-5
    ts = torch.full((x.shape[0], 1), 0.37)
    assert rel_l2(net(None, x, ts, b0, b1).numpy(), g["drift_1"]) <= 1e-5


def _adw1_pair():
    """(engine from ti_adw_create, engine from ti_adw_create_nd with dim = 1) on the adw_h256 weights."""
    ti = pkg()
    g = load_golden("adw_h256")
    H, L = int(g["hidden"]), int(g["num_layers"])
    flat = ti.weights.flatten_state_dict(ti.synthetic.adw_state_dict(H, L, int(g["seed"])), ti.weights.adw_param_spec(H, L), dtype=np.float64)
    e1 = ti.engine.AdwEngine(H, L, flat)
    e2 = ti.engine.AdwEngine(H, L, flat)
    w = np.ascontiguousarray(flat, np.float64)
    lib = ti._lib.lib()
    h = lib.ti_adw_create_nd(C.byref(e2.desc), 1, w.ctypes.data_as(C.POINTER(C.c_double)), w.size, 0)
    assert h
    lib.ti_destroy(e2.h)
    e2.h = h
    return g, e1, e2


def test_dim1_handle_is_bit_identical():
    g, e1, e2 = _adw1_pair()
    x = g["x"].astype(F32)
    b0, b1 = g["beta0_var"].astype(F32), g["beta1_var"].astype(F32)
    for a, b in zip(e1.drift(x, 0.3, b0, b1, return_div=True), e2.drift(x, 0.3, b0, b1, return_div=True)):
        np.testing.assert_array_equal(a, b)
    tv = np.linspace(0, 1, x.size).astype(F32)
    for a, b in zip(e1.drift(x, tv, b0, b1, return_div=True), e2.drift(x, tv, b0, b1, return_div=True)):
        np.testing.assert_array_equal(a, b)
    grid = np.linspace(0, 1, 6).astype(F32)
    for kw in (dict(scheme="em", eps=0.3, seed=7), dict(scheme="heun", return_dlogp=True), dict(scheme="dopri5", return_dlogp=True),
               dict(scheme="dopri5", return_dlogp=True, step_control="trajectory")):
        r1, r2 = e1.rollout(x, b0, b1, grid, **kw), e2.rollout(x, b0, b1, grid, **kw)
        for a, b in zip(r1, r2):
            np.testing.assert_array_equal(a, b)


def test_em_eps0_is_euler_and_noise_is_per_particle():
    g, sd = load_case("adw_nd3_h256")
    eng = _engine(g, sd)
    x, b0, b1 = g["x"].astype(F32), g["beta0"].astype(F32), g["beta1"].astype(F32)
    grid = np.linspace(0, 1, 9).astype(F32)
    np.testing.assert_array_equal(eng.rollout(x, b0, b1, grid, scheme="em", eps=0.0)[0], eng.rollout(x, b0, b1, grid, scheme="euler")[0])
    full, _ = eng.rollout(x, b0, b1, grid, scheme="em", eps=0.2, seed=5)
    assert np.isfinite(full).all() and np.abs(full[-1] - eng.rollout(x, b0, b1, grid, scheme="euler")[0][-1]).max() > 1e-3
    for b in (0, 17, x.shape[0] - 1):
        alone, _ = eng.rollout(x[b:b + 1], b0[b:b + 1], b1[b:b + 1], grid, scheme="em", eps=0.2, seed=5, traj_offset=b)
        np.testing.assert_array_equal(alone[:, 0], full[:, b])


@pytest.mark.parametrize("dlogp", [False, True])
def test_dopri5_batch_vs_odeint(dlogp):
    g, sd = load_case("adw_nd2_h64")
    eng = _engine(g, sd)
    x, b0, b1 = g["x"].astype(F32), g["beta0"].astype(F32), g["beta1"].astype(F32)
    grid = np.linspace(0, 1, 5).astype(F32)
    res = eng.rollout(x, b0, b1, grid, scheme="dopri5", return_dlogp=dlogp, rtol=1e-5, atol=1e-5)

    def own(t, y):
        b, div = eng.drift(np.ascontiguousarray(y[0], F32), t, b0, b1, return_div=True)
        return [b, (-div * F32(1e-2)).astype(F32)] if dlogp else [b]

    def fp64(t, y):
        b, div = np_drift(sd, y[0], t, b0, b1, return_div=True)
        return [b.astype(F32), (-div * 1e-2).astype(F32)] if dlogp else [b.astype(F32)]

    y0 = [x, np.zeros(x.shape[0], F32)] if dlogp else [x]
    sol, nfe = ode.odeint(own, y0, grid, "dopri5", 1e-5, 1e-5)
    assert res[-1] == nfe
    assert np.abs(res[0][-1] - sol[0][-1]).max() <= 1e-5 * max(1.0, np.abs(sol[0][-1]).max())
    if dlogp:
        assert np.abs(res[1][-1] - sol[1][-1] * 1e2).max() <= 1e-5 * max(1.0, np.abs(sol[1][-1] * 1e2).max())
    sol64, _ = ode.odeint(fp64, y0, grid, "dopri5", 1e-5, 1e-5)
    assert rel_l2(res[0][-1], sol64[0][-1]) <= 1e-4
    if dlogp:          # the dlogp state (before * 1e2) is of the size of atol: the two solves agree to atol, not relatively
        assert np.abs(res[1][-1] * 1e-2 - sol64[1][-1]).max() <= 1e-5


@pytest.mark.parametrize("dlogp", [False, True])
def test_dopri5_trajectory_mode(dlogp):
    g, sd = load_case("adw_nd3_h256")
    eng = _engine(g, sd)
    B = 12
    x = (g["x"][:B] * np.linspace(0.3, 3.0, B)[:, None]).astype(F32)
    b0, b1 = g["beta0_var"][:B].astype(F32), g["beta1_var"][:B].astype(F32)
    grid = np.linspace(0, 1, 4).astype(F32)
    kw = dict(scheme="dopri5", step_control="trajectory", return_dlogp=dlogp, rtol=1e-5, atol=1e-5)
    res = eng.rollout(x, b0, b1, grid, **kw)
    acc, rej = eng.step_counts(B)
    for b in range(B):
        alone = eng.rollout(x[b:b + 1], b0[b:b + 1], b1[b:b + 1], grid, **kw)
        for a, c in zip(res[:-1], alone[:-1]):
            np.testing.assert_array_equal(a[:, b], c[:, 0])
        sb0, sb1 = b0[b:b + 1], b1[b:b + 1]

        def own(t, y):
            o, div = eng.drift(np.ascontiguousarray(y[0], F32), t, sb0, sb1, return_div=True)
            return [o, (-div * F32(1e-2)).astype(F32)] if dlogp else [o]

        def fp64(t, y):
            o, div = np_drift(sd, y[0], t, sb0, sb1, return_div=True)
            return [o.astype(F32), (-div * 1e-2).astype(F32)] if dlogp else [o.astype(F32)]

        y0 = [x[b:b + 1], np.zeros(1, F32)] if dlogp else [x[b:b + 1]]
        sol, nfe = ode.odeint(own, y0, grid, "dopri5", 1e-5, 1e-5)
        assert acc[b] + rej[b] == (nfe - 2) // 6, b
        assert np.abs(res[0][-1, b] - sol[0][-1, 0]).max() <= 1e-5 * max(1.0, np.abs(sol[0][-1]).max())
        sol64, _ = ode.odeint(fp64, y0, grid, "dopri5", 1e-5, 1e-5)
        assert rel_l2(res[0][-1, b], sol64[0][-1, 0]) <= 1e-4
        if dlogp:      # as in the batch test: the dlogp state is of the size of atol
            assert abs(res[1][-1, b] * 1e-2 - sol64[1][-1, 0]) <= 1e-5


def test_device_memory_path_equals_host_path():
    torch = pytest.importorskip("torch")
    g, sd = load_case("adw_nd16_h128")
    eng = _engine(g, sd)
    x, b0, b1 = g["x"].astype(F32), g["beta0_var"].astype(F32), g["beta1_var"].astype(F32)
    dev = lambda a: torch.from_numpy(a).cuda()
    hb, hd = eng.drift(x, 0.37, b0, b1, return_div=True)
    db, dd = eng.drift(dev(x), 0.37, dev(b0), dev(b1), return_div=True)
    assert db.is_cuda and tuple(db.shape) == x.shape
    np.testing.assert_array_equal(db.cpu().numpy(), hb)
    np.testing.assert_array_equal(dd.cpu().numpy(), hd)
    grid = np.linspace(0, 1, 6).astype(F32)
    for kw in (dict(scheme="heun", return_dlogp=True), dict(scheme="dopri5", step_control="trajectory", return_dlogp=True)):
        rh = eng.rollout(x, b0, b1, grid, **kw)
        rd = eng.rollout(dev(x), dev(b0), dev(b1), grid, **kw)
        for a, c in zip(rh[:-1], rd[:-1]):
            assert c.is_cuda
            np.testing.assert_array_equal(c.cpu().numpy(), a)


def test_full_batch_d16_h256_em_is_finite_and_reproducible():
    ti = pkg()
    d, H, L, B = 16, 256, 5, 262144
    flat = ti.weights.flatten_state_dict(ti.synthetic.make_state_dict(ti.weights.adw_param_spec(H, L, d, d), seed=21, dtype=np.float64),
                                         ti.weights.adw_param_spec(H, L, d, d), dtype=np.float64)
    eng = ti.engine.AdwEngine(H, L, flat, dim=d)
    x = np.random.RandomState(0).standard_normal((B, d)).astype(F32)
    b0, b1 = np.full(B, 1.0, F32), np.full(B, 1.25, F32)
    grid = np.linspace(0, 1, 4).astype(F32)
    a, _ = eng.rollout(x, b0, b1, grid, scheme="em", eps=0.1, seed=3, save_every=0)
    assert a.shape == (1, B, d) and np.isfinite(a).all()
    again, _ = eng.rollout(x, b0, b1, grid, scheme="em", eps=0.1, seed=3, save_every=0)
    np.testing.assert_array_equal(again, a)
