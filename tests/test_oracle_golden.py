"""The CPU oracle (oracle/ti_oracle.c) against golden vectors produced by the reference's own PyTorch modules
(tests/golden/make_golden.py).  This is what pins the oracle; the GPU parity tests then use the oracle as checker."""
import numpy as np
import pytest

from conftest import golden_weights, load_golden, pkg, rel_l2
from oracle import oracle

PAINN_CASES = ["ambient_small", "ambient_sparse", "ambient_a9", "ambient_a25", "ambient_full", "ambient_ctor", "ambient_b1",
               "latent_multi", "latent_single", "latent_full", "latent_ctor",
               "range_big", "range_big_f128", "range_tiny", "range_tiny_f128", "range_close", "range_latent_big",
               "lnaff_1em5_f32", "lnaff_1em5_f128", "lnaff_1em3_f32", "lnaff_1em3_f128", "lnaff_1e3_f32", "lnaff_1e3_f128",
               "lnaff_harsh_f32", "lnaff_harsh_f128", "lnaff_zero_w_f32",
               "ambient_f256", "ambient_f256_taps", "latent_f256", "range_big_f256", "range_tiny_f256", "lnaff_1em5_f256", "lnaff_harsh_f256",
               "lnaff_zero_phi0_f32", "lnaff_zero_phi0_bigp_f32"]
# fp32 tolerance.  SURVEY.md §8c proposed 1e-6, but the reference's own fp32 forward sits 0.4e-6 (F=32) to 6e-6
# (latent, F=128, unit-variance coordinates) away from exact arithmetic (the oracle's fp64 mode) because of GEMM summation
# order and sin/cos of large arguments; two fp32 evaluations cannot agree better than that.  So: below the north-star bar
# (1e-5) and within 3x of the reference's own distance to exact arithmetic.
TOL_BAR = 1e-5


def close_f32(err32, err64):
    return err32 < TOL_BAR and err32 < 3.0 * max(err64, 5e-7)


def make_oracle(g):
    return oracle.PainnOracle(int(g["variant"]), int(g["F"]), int(g["L"]), int(g["A"]), g["edge_src"], g["edge_dst"], g["edge_type"],
                              g["atom_ids"], golden_weights(g), temp_length=float(g["temp_length"]), temperatures=g["temperatures"])


@pytest.mark.parametrize("name", PAINN_CASES)
def test_painn_drift_matches_reference(name):
    g = load_golden(name)
    o = make_oracle(g)
    for i, t in enumerate(g["ts"]):
        got = o.drift(g["x"], float(t), g["cond"])
        got64 = o.drift(g["x"], float(t), g["cond"], precision=64)
        e32, e64 = rel_l2(got, g[f"drift_{i}"]), rel_l2(got64, g[f"drift_{i}"])
        assert e64 < TOL_BAR, (name, i, e64)                  # reference fp32 round-off vs exact arithmetic
        assert close_f32(e32, e64), (name, i, e32, e64)


@pytest.mark.parametrize("name", ["ambient_small", "ambient_sparse", "latent_multi", "ambient_f256_taps"])
def test_painn_intermediates_match_reference(name):
    g = load_golden(name)
    o = make_oracle(g)
    B, A, F, L = int(g["B"]), int(g["A"]), int(g["F"]), int(g["L"])
    t = float(g["ts"][1])
    stages = [(0, "embed")] + [(1 + 2 * l, f"msg{l}") for l in range(L)] + [(2 + 2 * l, f"upd{l}") for l in range(L)]
    for stage, tag in stages:
        _, taps = o.drift(g["x"], t, g["cond"], tap_stage=stage)
        if tag == "embed":
            assert rel_l2(taps["s"].reshape(B * A, F), g["im::s_embed"]) < 3e-6
            continue
        assert rel_l2(taps["s"].reshape(B * A, F), g[f"im::s_{tag}"]) < 3e-6, tag
        assert rel_l2(taps["v"].reshape(B * A, F, 3), g[f"im::v_{tag}"]) < 2e-6, tag
        if tag.startswith("msg"):
            assert rel_l2(taps["e"].reshape(-1, F), g[f"im::e_{tag}"]) < 3e-6, tag


@pytest.mark.parametrize("name", ["ambient_small", "ambient_a9", "ambient_full", "latent_multi", "ambient_f256"])
@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_painn_fixed_step_trajectory(name, scheme):
    g = load_golden(name)
    o = make_oracle(g)
    path, nfe = o.rollout(g["x"], g["cond"], g["traj_grid"], scheme=scheme, save_every=1)
    ref = g[f"traj_{scheme}"]
    assert path.shape == ref.shape
    assert nfe == (len(g["traj_grid"]) - 1) * (2 if scheme == "heun" else 1)
    assert rel_l2(path - path[0], ref - ref[0]) < 5e-6      # displacement, not the (dominant) initial coordinates
    # save_every=0 returns only the end state; save_every=4 keeps rows 0,4,8,... plus the last
    last, _ = o.rollout(g["x"], g["cond"], g["traj_grid"], scheme=scheme, save_every=0)
    np.testing.assert_array_equal(last[0], path[-1])
    sub, _ = o.rollout(g["x"], g["cond"], g["traj_grid"], scheme=scheme, save_every=4)
    n = len(g["traj_grid"])
    rows = list(range(0, n, 4)) + ([n - 1] if (n - 1) % 4 else [])
    np.testing.assert_array_equal(sub, path[rows])


def test_em_eps0_is_euler_and_noise_is_standard_normal():
    g = load_golden("ambient_small")
    o = make_oracle(g)
    e, _ = o.rollout(g["x"], g["cond"], g["traj_grid"], scheme="euler")
    em, _ = o.rollout(g["x"], g["cond"], g["traj_grid"], scheme="em", eps=0.0, seed=3)
    np.testing.assert_array_equal(e, em)
    z = np.array([oracle.normal(7, tr, st, c) for tr in range(40) for st in range(10) for c in range(54)])
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02
    # counter-based: same key -> same value, different trajectory -> different stream
    assert oracle.normal(7, 5, 3, 2) == oracle.normal(7, 5, 3, 2) != oracle.normal(7, 6, 3, 2)


def adw_oracle(g):
    ti = pkg()
    H, nl = int(g["hidden"]), int(g["num_layers"])
    spec = ti.weights.adw_param_spec(H, nl)
    sd = {k[4:]: v for k, v in g.items() if k.startswith("sd::")} or ti.synthetic.adw_state_dict(H, nl, int(g["seed"]))
    return oracle.AdwOracle(H, nl, ti.weights.flatten_state_dict(sd, spec, dtype=np.float64))


@pytest.mark.parametrize("name", ["adw_h256", "adw_ctor_h64"])
def test_adw_drift_and_trajectory(name):
    g = load_golden(name)
    o = adw_oracle(g)
    for tag in ("", "_var"):
        b0, b1 = g["beta0" + tag], g["beta1" + tag]
        for i, t in enumerate(g["ts"]):
            got = o.drift(g["x"].astype(np.float64), float(t), b0, b1)
            assert rel_l2(got, g[f"drift{tag}_{i}"]) < 1e-12, (tag, i)          # fp64 vs fp64 reference
            got32 = o.drift(g["x"], float(t), b0, b1, precision=32)
            assert rel_l2(got32, g[f"drift{tag}_{i}"]) < 1e-5, (tag, i)         # fp32 arithmetic vs fp64 reference
    for scheme in ("euler", "heun"):
        path, _ = o.rollout(g["x"].astype(np.float64), g["beta0"], g["beta1"], g["traj_grid"], scheme=scheme)
        assert rel_l2(path, g[f"traj_{scheme}"]) < 1e-12


@pytest.mark.parametrize("name", ["adw_h256", "adw_ctor_h64"])
def test_adw_divergence_matches_reference_autograd(name):
    """ODEWrapper.compute_divergence (adw/thermo/models/ode_wrapper.py:55-67): the golden holds -div * 1e-2 from autograd."""
    g = load_golden(name)
    o = adw_oracle(g)
    for tag in ("", "_var"):
        b, div = o.drift_div(g["x"].astype(np.float64), 0.3, g["beta0" + tag], g["beta1" + tag])   # the generator used t = 0.3 (fp64)
        assert rel_l2(-div * 1e-2, g[f"negdiv{tag}_1"].ravel()) < 1e-10


# ------------------------------------------------------------------------------- mdqm9 exact divergence
DIV_CASES = ["div_ambient_small", "div_ambient_sparse", "div_ambient_f128", "div_latent_multi", "div_latent_single"]
# Tolerance for the divergence: the trace is a sum of 3A Jacobian entries of either sign, so rounding noise is measured
# against sum_k |J_kk| ~ the per-direction magnitudes, not against the (possibly cancelling) trace.  Stated bar: the fp32
# oracle and the fp32 reference autograd agree to 2e-5 * (|div| + 1) absolute on the unscaled divergence; the fp64 oracle
# shows what part of that is the reference's own round-off.
DIV_ATOL = 2e-5


@pytest.mark.parametrize("name", DIV_CASES)
def test_painn_divergence_matches_reference_autograd(name):
    g = load_golden(name)
    o = make_oracle(g)
    scale = float(g["div_scale"])
    ref_div = -g["negdiv_scaled"].astype(np.float64) / scale              # undo (b, -div * scale) of the wrapper
    b32, d32 = o.drift_div(g["x"], float(g["t"]), g["cond"], precision=32)
    b64, d64 = o.drift_div(g["x"], float(g["t"]), g["cond"], precision=64)
    assert rel_l2(b32, g["drift"]) < TOL_BAR and rel_l2(b64, g["drift"]) < TOL_BAR
    bar = DIV_ATOL * (np.abs(ref_div) + 1.0)
    assert (np.abs(d64 - ref_div) < bar).all(), (name, d64, ref_div)
    assert (np.abs(d32 - ref_div) < bar).all(), (name, d32, ref_div)
    # forward mode along an arbitrary direction agrees with a central difference of the fp64 drift
    rs = np.random.RandomState(3)
    h = np.float32(2.0 ** -11)
    xp = (g["x"] + h * rs.standard_normal(g["x"].shape)).astype(np.float32)
    xm = (2.0 * g["x"].astype(np.float64) - xp).astype(np.float32)
    xdot = ((xp.astype(np.float64) - xm) / (2.0 * float(h))).astype(np.float32)     # exact: the direction actually stepped in fp32
    _, tan = o.jvp(g["x"], xdot, float(g["t"]), g["cond"], precision=64)
    fd = (o.drift(xp, float(g["t"]), g["cond"], precision=64).astype(np.float64) - o.drift(xm, float(g["t"]), g["cond"], precision=64)) / (2.0 * float(h))
    assert rel_l2(tan, fd) < 1e-3              # O(h^2) truncation + fp32 storage of the drift (6e-8 / h)


@pytest.mark.parametrize("name", DIV_CASES)
@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_painn_dlogp_trajectory(name, scheme):
    """Two-state fixed-step loops over the reference ODEWrapper(return_dlogp=True): forward, and reverse_ode (latent)."""
    g = load_golden(name)
    o = make_oracle(g)
    scale = float(g["div_scale"])
    for rev in ([False, True] if "grid_rev" in g else [False]):
        tag = scheme + ("_rev" if rev else "")
        grid = g["grid_rev" if rev else "grid"]
        path, dl, nfe = o.rollout_dlogp(g["x"], g["cond"], grid, scheme=scheme, div_scale=scale, reverse_ode=rev)
        ref, ref_dl = g[f"traj_{tag}"], g[f"dlogp_{tag}"]
        assert path.shape == ref.shape and dl.shape == ref_dl.shape
        assert nfe == (len(grid) - 1) * (2 if scheme == "heun" else 1)
        assert rel_l2(path - path[0], ref - ref[0]) < 5e-6
        assert (np.abs(dl - ref_dl) < DIV_ATOL * scale * (np.abs(ref_dl) / scale + 1.0)).all(), (name, tag, dl, ref_dl)
        last, dl_last, _ = o.rollout_dlogp(g["x"], g["cond"], grid, scheme=scheme, save_every=0, div_scale=scale, reverse_ode=rev)
        np.testing.assert_array_equal(last[0], path[-1])
        np.testing.assert_array_equal(dl_last[0], dl[-1])


@pytest.mark.parametrize("name", ["div_ambient_full", "div_ambient_f256"])
def test_painn_divergence_headline_shape_matches_reference_autograd(name):
    """F = 128, L = 5, A = 18 (the bench shape) and F = 256, L = 5, A = 25 (the mdqm9 configs), one molecule: 54 / 75 reference
    double-backward passes vs as many oracle forward-mode passes.  fp32 oracle only (the fp64 pass and the rollouts of this size are
    left to the GPU suite: ~30 s each on 8 cores)."""
    g = load_golden(name)
    o = make_oracle(g)
    scale = float(g["div_scale"])
    ref_div = -g["negdiv_scaled"].astype(np.float64) / scale
    b32, d32 = o.drift_div(g["x"], float(g["t"]), g["cond"], precision=32)
    assert rel_l2(b32, g["drift"]) < TOL_BAR
    assert (np.abs(d32 - ref_div) < DIV_ATOL * (np.abs(ref_div) + 1.0)).all(), (d32, ref_div)


@pytest.mark.parametrize("name", ["lnaff_zero_phi0_f32", "lnaff_zero_phi0_bigp_f32", "lnaff_1em5_f256", "lnaff_harsh_f256"])
def test_lnaff_fixtures_reach_their_magnitudes(name):
    """The fixture-side check of the GPU magnitude tests (test_gpu_parity.check_lnaff_magnitudes), here without a GPU."""
    from test_gpu_parity import check_lnaff_magnitudes
    check_lnaff_magnitudes(name, load_golden(name))
