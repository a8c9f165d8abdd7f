"""The fused adw rollout (ti_adw_rollout_fused: the whole Euler / Heun / EM step loop in one kernel launch) on the GPU.

The contract is bit-identity with the host-driven rollout: `equal` below is np.array_equal on the raw arrays (path, dlogp) and
n_fevals.  Independent of the unfused code it is also held against the reference goldens and the fp64 oracle at the bars the unfused
tests use.  Needs a real MI355X: `pytest -m gpu`."""
import itertools

import numpy as np
import pytest

from conftest import load_golden, pkg, rel_l2
from oracle import oracle

pytestmark = pytest.mark.gpu

DRIFT_TOL = 1e-5          # tests/test_gpu_parity.py
N_STEP = 8
# (scheme, return_dlogp, eps, seed)
SCHEMES = [("euler", False, 0.0, 0), ("euler", True, 0.0, 0), ("heun", False, 0.0, 0), ("heun", True, 0.0, 0), ("em", False, 0.1, 5),
           ("em", False, 0.0, 5)]


def _flat(H, L, seed=0, dim=1):
    ti = pkg()
    spec = ti.weights.adw_param_spec(H, L, dim, dim)
    return ti.weights.flatten_state_dict(ti.synthetic.make_state_dict(spec, seed=seed, dtype=np.float64), spec, dtype=np.float64)


def _engine(H, L, precision="f32"):
    ti = pkg()
    flat = ti.weights.flatten_state_dict(ti.synthetic.adw_state_dict(H, L, H + L), ti.weights.adw_param_spec(H, L), dtype=np.float64)
    return ti.engine.AdwEngine(H, L, flat, precision=precision)


def _betas(B, pairs):
    """two distinct (beta0, beta1) pairs interleaved over the batch, or a single pair"""
    if pairs == 1:
        return np.full(B, 1.0, np.float32), np.full(B, 1.25, np.float32)
    i = np.arange(B) % 2
    return np.where(i == 0, 1.0, 0.75).astype(np.float32), np.where(i == 0, 1.25, 1.5).astype(np.float32)


def _both(eng, x, b0, b1, grid, **kw):
    """(unfused result, fused result) of the same call, as tuples of host arrays and n_fevals"""
    return eng.rollout(x, b0, b1, grid, **kw), eng.rollout(x, b0, b1, grid, fused=True, **kw)


def assert_equal(got, ref, what):
    assert len(got) == len(ref), what
    for g, r in zip(got[:-1], ref[:-1]):
        assert g.shape == r.shape and g.dtype == r.dtype, what
        assert np.array_equal(g, r), (what, int((g != r).sum()), float(np.abs(g - r).max()))
    assert got[-1] == ref[-1], what


# ------------------------------------------------------------------------------ 1. every instantiation, bit for bit
@pytest.mark.parametrize("H,L,precision", [(H, 3, p) for H in (32, 64, 128, 256) for p in ("f32", "f16x2")] +
                         [(32, 1, "f32"), (32, 1, "f16x2")])        # L = 1: the smallest ti_adw_create accepts (no hidden layer, no ring)
def test_fused_equals_unfused_bit_for_bit(H, L, precision):
    """B = 150: three workgroups, the last with one full wave, one wave of 6 rows and two waves without rows; B = 1.  save_every 3 on
    7 steps: the last row is not a multiple."""
    ti = pkg()
    eng = _engine(H, L, precision)
    grid = ti.engine.time_grid(0.0, 1.0, N_STEP)
    x_all = ti.synthetic.adw_x0(150, 1)
    for B, pairs, save_every in itertools.product((150, 1), (2, 1), (0, 1, 3)):
        x = x_all[:B]
        b0, b1 = _betas(B, pairs)
        fused = {}
        for scheme, dlogp, eps, seed in SCHEMES:
            ref, got = _both(eng, x, b0, b1, grid, scheme=scheme, save_every=save_every, eps=eps, seed=seed, return_dlogp=dlogp)
            what = (H, L, precision, B, pairs, save_every, scheme, dlogp, eps)
            rows = {0: 1, 1: N_STEP, 3: 4}[save_every]
            assert got[0].shape == (rows, B) and got[-1] == (N_STEP - 1) * (2 if scheme == "heun" else 1), what
            assert np.isfinite(got[0]).all(), what
            assert_equal(got, ref, what)
            fused[(scheme, dlogp, eps)] = got
        assert np.array_equal(fused[("em", False, 0.0)][0], fused[("euler", False, 0.0)][0])      # eps = 0 reproduces Euler
        assert not np.array_equal(fused[("em", False, 0.1)][0][-1], fused[("euler", False, 0.0)][0][-1])     # the noise is there
        for scheme in ("euler", "heun"):                                    # the dlogp state does not perturb the trajectory
            assert np.array_equal(fused[(scheme, True, 0.0)][0], fused[(scheme, False, 0.0)][0]), (H, L, precision, scheme)
            dl = fused[(scheme, True, 0.0)][1]
            assert np.isfinite(dl).all() and (save_every == 0 or not dl[0].any()) and dl[-1].any()


# ------------------------------------------------------------------------------ 2. counters and direction
@pytest.fixture(scope="module")
def eng64():
    return _engine(64, 3)


def test_noise_counters_follow_traj_and_step_offset(eng64):
    ti = pkg()
    B = 150
    x, (b0, b1) = ti.synthetic.adw_x0(B, 2), _betas(B, 2)
    grid = ti.engine.time_grid(0.0, 1.0, N_STEP)
    kw = dict(scheme="em", eps=0.1, seed=5, traj_offset=1000, step_offset=5)
    ref, got = _both(eng64, x, b0, b1, grid, **kw)
    assert_equal(got, ref, kw)
    plain = eng64.rollout(x, b0, b1, grid, scheme="em", eps=0.1, seed=5, fused=True)
    assert not np.array_equal(plain[0][1], got[0][1])                        # the offsets reach the counter


def test_two_chained_fused_calls_equal_one_unfused_call(eng64):
    ti = pkg()
    B = 150
    x, (b0, b1) = ti.synthetic.adw_x0(B, 3), _betas(B, 2)
    grid = ti.engine.time_grid(0.0, 1.0, 9)
    whole, nfe = eng64.rollout(x, b0, b1, grid, scheme="em", eps=0.1, seed=7)
    first, n1 = eng64.rollout(x, b0, b1, grid[:5], scheme="em", eps=0.1, seed=7, fused=True)
    second, n2 = eng64.rollout(first[-1].copy(), b0, b1, grid[4:], scheme="em", eps=0.1, seed=7, step_offset=4, fused=True)
    assert np.array_equal(np.concatenate([first, second[1:]]), whole) and n1 + n2 == nfe


def test_decreasing_grid(eng64):
    ti = pkg()
    B = 150
    x, (b0, b1) = ti.synthetic.adw_x0(B, 4), _betas(B, 2)
    grid = ti.engine.time_grid(1.0, 0.0, N_STEP)
    for kw in (dict(scheme="euler", return_dlogp=True), dict(scheme="em", eps=0.1, seed=5)):
        ref, got = _both(eng64, x, b0, b1, grid, **kw)
        assert_equal(got, ref, kw)


# ------------------------------------------------------------------------------ 3. memory kinds
def test_host_arrays_and_cuda_tensors_agree(eng64):
    torch = pytest.importorskip("torch")
    ti = pkg()
    B = 150
    x, (b0, b1) = ti.synthetic.adw_x0(B, 5), _betas(B, 2)
    grid = ti.engine.time_grid(0.0, 1.0, N_STEP)
    xd, b0d, b1d = (torch.from_numpy(a).cuda() for a in (x, b0, b1))
    for kw in (dict(scheme="heun", return_dlogp=True, save_every=3), dict(scheme="em", eps=0.1, seed=5, save_every=0)):
        host = eng64.rollout(x, b0, b1, grid, fused=True, **kw)
        dev = eng64.rollout(xd, b0d, b1d, grid, fused=True, **kw)
        assert all(t.is_cuda for t in dev[:-1])
        assert_equal(tuple(t.cpu().numpy() for t in dev[:-1]) + (dev[-1],), host, kw)
        assert_equal(host, eng64.rollout(x, b0, b1, grid, **kw), kw)
    # out= is filled in place, on either side
    out = np.full((N_STEP, B), np.nan, np.float32)
    res, _ = eng64.rollout(x, b0, b1, grid, scheme="euler", out=out, fused=True)
    assert res is out and np.array_equal(out, eng64.rollout(x, b0, b1, grid, scheme="euler")[0])
    outd = torch.full((N_STEP, B), float("nan"), device="cuda")
    resd, _ = eng64.rollout(xd, b0d, b1d, grid, scheme="euler", out=outd, fused=True)
    assert resd is outd and np.array_equal(outd.cpu().numpy(), out)


# ------------------------------------------------------------------------------ 4. independent of the unfused code
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_fused_vs_reference_golden_and_oracle(precision):
    """golden adw_h256: the bars of test_adw_drift_and_rollout_vs_reference and test_adw_divergence_and_dlogp (tests/test_gpu_parity.py)"""
    ti = pkg()
    g = load_golden("adw_h256")
    H, nl = int(g["hidden"]), int(g["num_layers"])
    sd = {k[4:]: v for k, v in g.items() if k.startswith("sd::")} or ti.synthetic.adw_state_dict(H, nl, int(g["seed"]))
    flat = ti.weights.flatten_state_dict(sd, ti.weights.adw_param_spec(H, nl), dtype=np.float64)
    eng, orc = ti.engine.AdwEngine(H, nl, flat, precision=precision), oracle.AdwOracle(H, nl, flat)
    b0, b1 = g["beta0"].astype(np.float32), g["beta1"].astype(np.float32)
    for scheme in ("euler", "heun"):
        if precision == "f32":                  # the golden bar is the fp32 path's, as in test_adw_drift_and_rollout_vs_reference
            path, nfe = eng.rollout(g["x"], b0, b1, g["traj_grid"], scheme=scheme, fused=True)
            ref = g[f"traj_{scheme}"]
            assert path.shape == ref.shape
            assert rel_l2(path - path[0], ref - ref[0]) < 2e-5, scheme
        x, dl, nfe = eng.rollout(g["x"], b0, b1, g["traj_grid"], scheme=scheme, return_dlogp=True, fused=True)
        xr, dlr, _ = orc.rollout(g["x"].astype(np.float64), b0, b1, g["traj_grid"], scheme=scheme, return_dlogp=True)
        assert x.shape == dl.shape == xr.shape and np.all(dl[0] == 0)
        assert rel_l2(x, xr) < DRIFT_TOL and rel_l2(dl, dlr) < 2e-5, (scheme, precision)
    if precision != "f32":
        return
    em, _ = eng.rollout(g["x"], b0, b1, g["traj_grid"], scheme="em", eps=0.1, seed=5, fused=True)
    ref, _ = orc.rollout(g["x"].astype(np.float64), b0, b1, g["traj_grid"], scheme="em", eps=0.1, seed=5)
    assert rel_l2(em, ref) < 1e-4, precision


# ------------------------------------------------------------------------------ 5. it really is fused
def test_fused_rollout_takes_two_launches(eng64):
    ti = pkg()
    B = 150
    x, (b0, b1) = ti.synthetic.adw_x0(B, 6), _betas(B, 2)
    grid = ti.engine.time_grid(0.0, 1.0, 50)
    eng64.profile(True)
    try:
        eng64.profile_read("adw"), eng64.profile_read("integrate")          # reading clears the slots
        got = eng64.rollout(x, b0, b1, grid, scheme="euler", save_every=0, fused=True)
        assert eng64.profile_read("adw")[0] == 2 and eng64.profile_read("integrate")[0] == 0
        ref = eng64.rollout(x, b0, b1, grid, scheme="euler", save_every=0)
        assert eng64.profile_read("adw")[0] == 98 and eng64.profile_read("integrate")[0] == 49
    finally:
        eng64.profile(False)
    assert_equal(got, ref, "n_step = 50")


# ------------------------------------------------------------------------------ 6. refusals on a live handle
def test_refusals_leave_the_handle_usable():
    ti = pkg()
    UNSUPPORTED = ti._lib.TI_E_UNSUPPORTED
    B = 20
    grid = ti.engine.time_grid(0.0, 1.0, N_STEP)
    b0, b1 = _betas(B, 2)
    nd = ti.engine.AdwEngine(32, 2, _flat(32, 2, dim=2), dim=2)
    with pytest.raises(ti._lib.TiError, match="ti_adw_rollout") as e:
        nd.rollout(np.zeros((B, 2), np.float32), b0, b1, grid, scheme="euler", fused=True)
    assert e.value.code == UNSUPPORTED
    assert np.isfinite(nd.rollout(np.zeros((B, 2), np.float32), b0, b1, grid, scheme="euler")[0]).all()

    eng = _engine(64, 3)
    x = ti.synthetic.adw_x0(B, 7)
    refused = [dict(scheme="midpoint"), dict(scheme="rk4"), dict(scheme="dopri5"), dict(scheme="dopri5", step_control="trajectory"),
               dict(scheme="em", eps=0.1, return_dlogp=True)]
    for kw in refused:
        with pytest.raises(ti._lib.TiError) as e:
            eng.rollout(x, b0, b1, grid, fused=True, **kw)
        assert e.value.code == UNSUPPORTED, kw
    cv = np.zeros((N_STEP, B, 1), np.float32)
    eng.set_observer([("coord", 0)], every=1, out=cv)
    try:
        with pytest.raises(ti._lib.TiError, match="observer") as e:
            eng.rollout(x, b0, b1, grid, scheme="euler", fused=True)
        assert e.value.code == UNSUPPORTED and not cv.any()
    finally:
        eng.set_observer(None)
    ref, got = _both(eng, x, b0, b1, grid, scheme="heun", return_dlogp=True)
    assert_equal(got, ref, "after the refusals")


# ------------------------------------------------------------------------------ 7. mirror class
def test_standard_integrator_fused():
    torch = pytest.importorskip("torch")
    ti = pkg()
    g = load_golden("adw_ctor_h64")
    net = ti.thermo.adw.FCNetMultiBeta(1, 1, int(g["hidden"]), int(g["num_layers"]))
    net.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd::")})
    x0s = torch.from_numpy(g["x"])[:, None]
    beta0s = torch.from_numpy(g["beta0"])[:, None]
    beta1s = torch.ones_like(beta0s) * 1.25
    n_step = len(g["traj_grid"])
    res = {}
    for fused in (False, True):
        integ = ti.thermo.adw.StandardIntegrator(b=net, method="heun", rtol=1e-4, atol=1e-4, n_step=n_step, return_dlogp=True, fused=fused)
        sample, dlogp = integ.rollout(x0s, beta0s=beta0s, beta1s=beta1s)
        assert tuple(sample.shape) == tuple(dlogp.shape) == (n_step, len(g["x"]), 1) and integ.n_fevals == 2 * (n_step - 1)
        res[fused] = (sample.numpy(), dlogp.numpy())
    assert np.array_equal(res[True][0], res[False][0]) and np.array_equal(res[True][1], res[False][1])
    assert rel_l2(res[True][0][:, :, 0], g["traj_heun"]) < 1e-5
    with pytest.raises(TypeError):
        ti.thermo.adw.StandardIntegrator(net, "heun", n_step, 1e-4, 1e-4, 0.0, 1.0, True, True)          # fused is keyword-only
