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


# ------------------------------------------------------------------------------- exact divergence at the magnitude edges
# The drift's range_* / lnaff_* recipes, evaluated by the reference's double backward (make_golden.py div_range_cases).  Not in
# DIV_CASES: their divergences run from 1e-9 to 1e10, so neither the `+ 1` floor of DIV_ATOL nor a fixed absolute bar means anything.
DIV_RANGE_CASES = ["div_range_big", "div_range_big_f128", "div_range_tiny", "div_range_tiny_f128", "div_range_close",
                   "div_range_latent_big", "div_lnaff_1em5_f32", "div_lnaff_harsh_f128", "div_lnaff_zero_w_f32",
                   "div_lnaff_zero_phi0_bigp_f32", "div_range_big_f256", "div_lnaff_harsh_f256"]
# the cases whose Euler / Heun loops stay meaningful (range_big's drift throws its atoms to |x| ~ 1e5 in one step)
DIV_RANGE_TRAJ = ["div_range_tiny", "div_lnaff_1em5_f32"]
# relative bar against the case's own scale S = sum_i |d b_i / d x_i| (a trace of 3A entries of either sign rounds like S, not like it)
DIV_REL = 2e-5


def divergence_scale(o, g, precision=64):
    """S [B] = sum_i |J_ii| from unit-seed JVPs of the oracle."""
    B, A, t = int(g["B"]), int(g["A"]), float(g["t"])
    S = np.zeros(B)
    for i in range(3 * A):
        e = np.zeros((B, A, 3), np.float32)
        e.reshape(B, -1)[:, i] = 1.0
        S += np.abs(o.jvp(g["x"], e, t, g["cond"], precision=precision)[1].reshape(B, -1)[:, i].astype(np.float64))
    return S


def unit_seed_tangent_taps(o, g):
    """{stream: [max |tangent| over the case per stage]} of the fp64 oracle's tangent taps (ts, tv, te after every message / update
    stage) along all 3A unit seeds."""
    B, A, L, t = int(g["B"]), int(g["A"]), int(g["L"]), float(g["t"])
    out = {k: np.zeros(2 * L) for k in ("s", "v", "e")}
    for i in range(3 * A):
        e = np.zeros((B, A, 3), np.float32)
        e.reshape(B, -1)[:, i] = 1.0
        for st in range(1, 2 * L + 1):
            _, _, taps = o.jvp(g["x"], e, t, g["cond"], precision=64, tap_stage=st)
            for k in out:
                out[k][st - 1] = max(out[k][st - 1], float(np.abs(taps[k]).max()))
    return out


@pytest.mark.parametrize("name", DIV_RANGE_CASES)
def test_painn_divergence_magnitude_edges_match_reference_autograd(name):
    g = load_golden(name)
    o = make_oracle(g)
    ref_div = -g["negdiv_scaled"].astype(np.float64) / float(g["div_scale"])
    b32, d32 = o.drift_div(g["x"], float(g["t"]), g["cond"], precision=32)
    b64, d64 = o.drift_div(g["x"], float(g["t"]), g["cond"], precision=64)
    S = divergence_scale(o, g)
    # exact arithmetic against the reference's fp32 autograd, on the case's own scale (not vacuous for |div| << 1)
    assert (np.abs(d64 - ref_div) < DIV_REL * S).all(), (name, d64, ref_div, S)
    # the fp32 oracle: within 3x the fp32 floor -- the larger of the two fp32 evaluations' distances to exact arithmetic -- or the
    # case's own DIV_REL * S (which takes the place of DIV_ATOL: an absolute 2e-5 would pass anything at |div| ~ 1e-9)
    floor = max(float(np.abs(ref_div - d64).max()), float(np.abs(d32 - d64).max()))
    bar = np.maximum(DIV_REL * S, 3.0 * floor)
    assert (np.abs(d32 - ref_div) < bar).all(), (name, d32, ref_div, bar)
    assert (bar < 0.1 * S).all(), (name, bar, S)
    assert np.isfinite(b32).all() and rel_l2(b64, g["drift"]) < TOL_BAR


@pytest.mark.parametrize("name", DIV_RANGE_TRAJ)
@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_painn_dlogp_trajectory_magnitude_edges(name, scheme):
    g = load_golden(name)
    o = make_oracle(g)
    scale = float(g["div_scale"])
    S = divergence_scale(o, g) * scale
    grid = g["grid"]
    path, dl, _ = o.rollout_dlogp(g["x"], g["cond"], grid, scheme=scheme, div_scale=scale, precision=64)
    ref, ref_dl = g[f"traj_{scheme}"], g[f"dlogp_{scheme}"]
    assert rel_l2(path - path[0], ref - ref[0]) < 5e-6
    # dlogp after k steps is a sum of k divergences of size ~S (dt <= 1): on that scale
    assert (np.abs(dl - ref_dl) < DIV_REL * S).all(), (name, dl, ref_dl, S)


@pytest.mark.parametrize("name", [n for n in DIV_RANGE_CASES if n.endswith(("_big", "_big_f128", "_big_f256")) or "_tiny" in n or "lnaff_1em5" in n or "lnaff_harsh" in n])
def test_div_range_fixtures_reach_their_magnitudes(name):
    """The cases reach what they claim: the tangents the tangent kernels split as operands (te, tv, ts along unit seeds) leave the
    fp16 range in the *_big cases (> 65504: an unscaled hi half is inf) and fall below 1e-7 in the *_tiny cases (an unscaled lo half is
    an fp16 subnormal).  In the LayerNorm-affine cases the LayerNorm outputs and their tangents are scaled by the 1e-5 affines, so the
    tangent rows that enter the next products are tiny, not large: the edge-feature tangent stays below 1e-7."""
    g = load_golden(name)
    mx = unit_seed_tangent_taps(make_oracle(g), g)
    top = max(float(v.max()) for v in mx.values())
    least = min(float(v.max()) for v in mx.values())
    if "_big" in name:
        assert top > 65504.0, (name, mx)
    elif "_tiny" in name:
        assert least < 1e-7, (name, mx)
    else:
        assert float(mx["e"].max()) < 1e-7, (name, mx)


# ------------------------------------------------------------------------------------------------------------ finite-cutoff graphs
MASK_CASES = ["mask_ambient", "mask_latent", "mask_ambient_f256", "mask_latent_f256"]


@pytest.mark.parametrize("name", MASK_CASES)
def test_painn_oracle_on_each_molecules_own_graph_matches_the_reference(name):
    """tests/golden/make_golden_mask.py: the reference's collated finite-cutoff batch (every molecule its own radius + bond graph).  The
    oracle, given each molecule's own edges, reproduces the reference's drift at every time and its compute_divergence (ambient: times
    ODEWrapper.DIV_SCALE) -- the per-molecule reference the masked GPU kernels are measured against."""
    ti = pkg()
    g = load_golden(name)
    variant, F, L, A, B = (int(g[k]) for k in ("variant", "F", "L", "A", "B"))
    flat = ti.weights.flatten_state_dict(ti.synthetic.painn_state_dict(variant, F, L, 25, int(g["seed"])),
                                         ti.weights.painn_param_spec(variant, F, L, 25))
    ei, et = g["edge_index"], g["edge_type"]
    mol = g["batch"][ei[0]]
    scale = (ti.thermo.ambient if variant == 0 else ti.thermo.latent).ODEWrapper.DIV_SCALE
    ref_div = g["div"].astype(np.float64) / scale
    sizes = set()
    for b in range(B):
        own = mol == b
        sizes.add(int(own.sum()))
        o = oracle.PainnOracle(variant, F, L, A, ei[0][own] - b * A, ei[1][own] - b * A, et[own], g["atom_ids"][b * A:(b + 1) * A], flat,
                               temp_length=float(g["temp_length"]), temperatures=g["temperatures"])
        xb, cb = g["x"][b:b + 1], g["cond"][b:b + 1]
        for i, t in enumerate(g["ts"]):
            ref = g[f"drift_{i}"][b:b + 1]
            e32, e64 = rel_l2(o.drift(xb, float(t), cb), ref), rel_l2(o.drift(xb, float(t), cb, precision=64), ref)
            assert e64 < TOL_BAR, (name, b, i, e64)
            assert close_f32(e32, e64), (name, b, i, e32, e64)
        _, d = o.drift_div(xb, float(g["div_t"]), cb, precision=64)
        assert abs(float(d[0]) - ref_div[b]) < DIV_ATOL * (abs(ref_div[b]) + 1.0), (name, b, float(d[0]), ref_div[b])
    assert len(sizes) > 1                                   # the molecules really have different graphs
