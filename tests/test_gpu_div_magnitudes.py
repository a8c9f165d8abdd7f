"""The exact divergence, its tangent kernels and the dlogp rollout at the magnitude edges the drift is pinned at (tests/golden/div_range_*,
div_lnaff_*: the range_* / lnaff_* recipes evaluated by the reference's double backward), against the fp64 oracle.

Bars.  A divergence is a trace of 3A Jacobian entries of either sign, so its rounding is measured against the case's own scale
S = sum_i |d b_i / d x_i| (from the fp64 oracle's unit-seed JVPs), not against |div| + 1: at |div| ~ 1e-9 an absolute 2e-5 passes any
answer.  |div - div64| < max(DIV_REL * S, 3 x the fp32 oracle's distance to fp64), and every test checks that its bar is below 10 % of S.
Tangents (rel-L2): max(TOL, 3 x the fp32 oracle's rel-L2 distance to fp64), as in test_gpu_f256.py.
The tangent kernels split every operand row that is not a LayerNorm output by a power of two of its maximum (primal e, V v, s and all
tangent rows), so a tangent 2^k xdot gives 2^k times the tangent bit for bit: checked in f32 for k in [-16, 16] and in f16x2 for
k in {-40, ..., 40}.
"""
import functools

import numpy as np
import pytest

from conftest import load_golden, rel_l2
from test_gpu_divergence import make_pair

pytestmark = pytest.mark.gpu

TOL = 1e-5
DIV_REL = 2e-5
CASES = ["div_range_big", "div_range_big_f128", "div_range_tiny", "div_range_tiny_f128", "div_range_close", "div_range_latent_big",
         "div_lnaff_1em5_f32", "div_lnaff_harsh_f128", "div_lnaff_zero_w_f32", "div_lnaff_zero_phi0_bigp_f32", "div_range_big_f256",
         "div_lnaff_harsh_f256"]
TRAJ_CASES = ["div_range_tiny", "div_lnaff_1em5_f32"]       # the cases whose Euler / Heun loops stay meaningful
SWEEP_CASES = ["div_ambient_small", "div_range_close", "div_lnaff_1em5_f32", "div_range_tiny"]


@functools.lru_cache(maxsize=None)
def _oracle_div(name):
    """(div64 [B], fp32 oracle's |div32 - div64| [B], S [B]) of a fixture."""
    g = load_golden(name)
    _, orc = make_pair(g)
    B, A, t = int(g["B"]), int(g["A"]), float(g["t"])
    _, d64 = orc.drift_div(g["x"], t, g["cond"], precision=64)
    _, d32 = orc.drift_div(g["x"], t, g["cond"], precision=32)
    S = np.zeros(B)
    for i in range(3 * A):
        e = np.zeros((B, A, 3), np.float32)
        e.reshape(B, -1)[:, i] = 1.0
        S += np.abs(orc.jvp(g["x"], e, t, g["cond"], precision=64)[1].reshape(B, -1)[:, i].astype(np.float64))
    return d64.astype(np.float64), np.abs(d32.astype(np.float64) - d64), S


def div_bar(name):
    d64, floor, S = _oracle_div(name)
    bar = np.maximum(DIV_REL * S, 3.0 * floor)
    assert (bar < 0.1 * S).all(), (name, bar, S)               # no case is vacuous
    return d64, bar


def tangent_bar(orc, x, xdot, t, cond, tap_stage=-1):
    """(fp64 oracle result, bar) for a JVP or its tangent taps."""
    if tap_stage < 0:
        r64 = orc.jvp(x, xdot, t, cond, precision=64)[1]
        r32 = orc.jvp(x, xdot, t, cond, precision=32)[1]
        return r64, max(TOL, 3.0 * rel_l2(r32, r64))
    t64 = orc.jvp(x, xdot, t, cond, precision=64, tap_stage=tap_stage)[2]
    t32 = orc.jvp(x, xdot, t, cond, precision=32, tap_stage=tap_stage)[2]
    return t64, {k: max(TOL, 3.0 * rel_l2(t32[k], t64[k])) for k in t64}


@pytest.mark.parametrize("template", ["throughput", "latency"])
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", CASES)
def test_divergence_magnitude_edges_vs_fp64_oracle(name, precision, template):
    g = load_golden(name)
    eng, _ = make_pair(g, precision)
    eng.set_template(template)
    d64, bar = div_bar(name)
    b, div = eng.drift_div(g["x"], float(g["t"]), g["cond"])
    assert np.isfinite(b).all() and np.isfinite(div).all(), (name, div)
    assert (np.abs(div - d64) < bar).all(), (name, div, d64, bar)
    np.testing.assert_array_equal(eng.drift_div(g["x"], float(g["t"]), g["cond"])[1], div)      # fixed summation order
    eng.close()


# (div_lnaff_zero_w_f32 in f16x2 is left out: its filter MLP's first matrix is 1e-15 times its usual size, and the tangent kernels keep
# their weights as unscaled fp16 (hi, lo) halves, in which such a matrix is zero.  The tangent it carries -- ts after the first message
# block, ~1e-27 -- is then lost, while every output it feeds stays within its bar: the divergence of that case is checked above.)
TAP_PARAMS = [(n, p) for n in CASES for p in ("f32", "f16x2") if (n, p) != ("div_lnaff_zero_w_f32", "f16x2")]


@pytest.mark.parametrize("name,precision", TAP_PARAMS)
def test_jvp_stage_taps_magnitude_edges_vs_fp64_oracle(name, precision):
    """ts, tv, te after every stage, so that a failure names the kernel that produced it."""
    g = load_golden(name)
    eng, orc = make_pair(g, precision)
    B, L, t, x, cond = int(g["B"]), int(g["L"]), float(g["t"]), g["x"], g["cond"]
    xdot = np.random.RandomState(5).standard_normal(x.shape).astype(np.float32)
    _, tan = eng.jvp(x, xdot, t, cond)
    ref, bar = tangent_bar(orc, x, xdot, t, cond)
    assert np.isfinite(tan).all() and rel_l2(tan, ref) < bar, (name, rel_l2(tan, ref), bar)
    try:
        for stage in range(1, 2 * L + 1):
            tag = f"msg{(stage - 1) // 2}" if stage % 2 else f"upd{(stage - 2) // 2}"
            eng.debug_tap(stage)
            eng.jvp(x, xdot, t, cond)
            taps, bars = tangent_bar(orc, x, xdot, t, cond, tap_stage=stage)
            got = {"s": eng.debug_read("ts", B), "v": eng.debug_read("tv", B).transpose(0, 1, 3, 2)}
            if tag.startswith("msg") and stage < 2 * L - 1:
                got["e"] = eng.debug_read("te", B)
            for k, v in got.items():
                err = rel_l2(v, taps[k])
                assert np.isfinite(v).all() and err < bars[k], (name, tag, "t" + k, err, bars[k])
    finally:
        eng.debug_tap(-1)
    eng.close()


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("scheme", ["euler", "heun"])
@pytest.mark.parametrize("name", TRAJ_CASES)
def test_dlogp_rollout_magnitude_edges_vs_fp64_oracle(name, scheme, precision):
    g = load_golden(name)
    eng, orc = make_pair(g, precision)
    scale = float(g["div_scale"])
    _, _, S = _oracle_div(name)
    path, dl, _ = eng.rollout_dlogp(g["x"], g["cond"], g["grid"], scheme=scheme, div_scale=scale)
    rpath, rdl, _ = orc.rollout_dlogp(g["x"], g["cond"], g["grid"], scheme=scheme, div_scale=scale, precision=64)
    assert rel_l2(path - path[0], rpath - rpath[0]) < 2e-5
    # dlogp after k steps of dt <= 1 sums k divergences of scale ~S
    bar = DIV_REL * S * scale
    assert (np.abs(dl - rdl) < bar).all(), (name, scheme, dl, rdl, bar)
    eng.close()


@pytest.mark.parametrize("name", SWEEP_CASES + ["div_range_big"])
def test_tangent_scale_sweep_f32_bit_exact(name):
    """jvp is linear in xdot: in fp32 every tangent operation commutes with a power of two, so jvp(x, 2^k xi) = 2^k jvp(x, xi) exactly."""
    g = load_golden(name)
    eng, _ = make_pair(g, "f32")
    x, t, cond = g["x"], float(g["t"]), g["cond"]
    xi = np.random.RandomState(9).standard_normal(x.shape).astype(np.float32)
    _, tan0 = eng.jvp(x, xi, t, cond)
    for k in range(-16, 17):
        _, tan = eng.jvp(x, np.ldexp(xi, k), t, cond)
        np.testing.assert_array_equal(tan, np.ldexp(tan0, k), err_msg=f"{name} k={k}")
    eng.close()


@pytest.mark.parametrize("name", SWEEP_CASES)
def test_tangent_scale_sweep_f16x2(name):
    """f16x2 at tangent scales far outside fp16's range: within the bar of the fp64 oracle at every scale, and bit-exactly
    2^k times the k = 0 tangent, because every tangent operand row is divided by the power of two of its own maximum before the split."""
    g = load_golden(name)
    eng, orc = make_pair(g, "f16x2")
    x, t, cond = g["x"], float(g["t"]), g["cond"]
    xi = np.random.RandomState(9).standard_normal(x.shape).astype(np.float32)
    _, tan0 = eng.jvp(x, xi, t, cond)
    ref0, bar = tangent_bar(orc, x, xi, t, cond)
    for k in (-40, -24, -12, 0, 12, 24, 40):
        _, tan = eng.jvp(x, np.ldexp(xi, k), t, cond)
        err = rel_l2(np.ldexp(tan.astype(np.float64), -k), ref0)
        assert np.isfinite(tan).all() and err < bar, (name, k, err, bar)
        np.testing.assert_array_equal(tan, np.ldexp(tan0, k), err_msg=f"{name} k={k}")
    eng.close()
