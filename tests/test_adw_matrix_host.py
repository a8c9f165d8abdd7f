"""The references of the adw instantiation matrix (tests/test_gpu_adw_matrix.py), without a GPU: the fp64 numpy restatement at d = 1
against the C oracle, so one reference serves every d; the plain float32 model inside the bars of every cell with 3x to spare, so the
bars are not already spent by the reference's own rounding; and the f16x2 weight check of ti_adw_create_nd, which runs before any
device call."""
import ctypes as C

import numpy as np
import pytest

from adw_nd_numpy import MATRIX, MODES, TAN_GROUP, cell_inputs, cell_reference, cell_state_dict, drift, mode_args
from conftest import load_golden, pkg, rel_l2
from oracle import oracle

BAR = 1e-5          # tests/test_gpu_adw_nd.py: drift and divergence rel-L2 against fp64


@pytest.mark.parametrize("name", ["adw_h256", "adw_ctor_h64"])
def test_restatement_at_d1_equals_the_c_oracle(name):
    ti = pkg()
    g = load_golden(name)
    H, L = int(g["hidden"]), int(g["num_layers"])
    spec = ti.weights.adw_param_spec(H, L)
    assert spec == ti.weights.adw_param_spec(H, L, 1, 1)
    sd = {k[4:]: v.astype(np.float64) for k, v in g.items() if k.startswith("sd::")} or ti.synthetic.adw_state_dict(H, L, int(g["seed"]))
    orc = oracle.AdwOracle(H, L, ti.weights.flatten_state_dict(sd, spec, dtype=np.float64))
    x = g["x"].astype(np.float64)
    for tag in ("", "_var"):
        b0, b1 = g["beta0" + tag], g["beta1" + tag]
        for t in g["ts"]:
            ob, od = orc.drift_div(x, float(t), b0, b1)
            b, div = drift(sd, x[:, None], float(t), b0, b1, return_div=True)
            assert b.shape == (x.size, 1)
            assert rel_l2(b[:, 0], ob) <= 1e-12, (tag, t)
            assert rel_l2(div, od) <= 1e-12, (tag, t)


@pytest.mark.parametrize("H,d,L", MATRIX)
def test_float32_model_meets_the_bars_with_3x_to_spare(H, d, L):
    for mode in MODES:
        b64, d64 = cell_reference(H, d, L, mode)
        b32, d32 = cell_reference(H, d, L, mode, True)
        assert b32.dtype == np.float32 and d32.dtype == np.float32
        eb, ed = rel_l2(b32, b64), rel_l2(d32, d64)
        assert 3 * eb <= BAR and 3 * ed <= BAR, (mode, eb, ed)


def test_matrix_reaches_every_tangent_grouping():
    """The cells this file relies on: per width a short group behind a full one, full groups only, and d = 1."""
    for H, G in TAN_GROUP.items():
        ds = {d for h, d, _ in MATRIX if h == H}
        assert 1 in ds and any(d > G and d % G for d in ds) == (G > 1) and any(d > 1 and d % G == 0 for d in ds), (H, sorted(ds))
        assert {1} < {L for h, _, L in MATRIX if h == H}


def test_peak_activation_is_the_largest_silu_output():
    sd = cell_state_dict(64, 3, 3)
    inp = cell_inputs(3, 48, False)
    t, b0, b1 = mode_args(inp, ("scalar", "rows"))
    b, div, peak = drift(sd, inp.x * np.float32(1e4), t, b0, b1, return_div=True, return_peak=True)
    b1x, peak1 = drift(sd, inp.x, t, b0, b1, return_peak=True)
    assert peak.shape == (48,) and (peak > 50 * peak1).all() and (peak1 > 0.1).all() and (peak1 < 10).all()
    np.testing.assert_array_equal(drift(sd, inp.x * np.float32(1e4), t, b0, b1), b)


# ------------------------------------------------------------------------------------------------ f16x2 weights at creation
@pytest.fixture(scope="module")
def lib():
    ti = pkg()
    ti.build.build()
    return ti._lib.lib()


def _create(lib, H, L, dim, w, precision, nd=True):
    ti = pkg()
    desc = ti._lib.AdwDesc(H, L, ti._lib.PRECISIONS[precision])
    p = w.ctypes.data_as(C.POINTER(C.c_double))
    return lib.ti_adw_create_nd(C.byref(desc), dim, p, w.size, 0) if nd else lib.ti_adw_create(C.byref(desc), p, w.size, 0)


@pytest.mark.parametrize("bad", [1e5, -65504.0, float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("H,L,dim", [(64, 3, 5), (32, 1, 1)])
def test_create_nd_refuses_f16x2_weights_outside_fp16(lib, H, L, dim, bad):
    ti = pkg()
    w = ti.weights.flatten_state_dict(cell_state_dict(H, L, dim), ti.weights.adw_param_spec(H, L, dim, dim), dtype=np.float64)
    for at in (0, w.size // 2, w.size - 1):
        v = w.copy()
        v[at] = bad
        assert not _create(lib, H, L, dim, v, "f16x2")
        msg = ti._lib.last_error()
        assert "65504" in msg and f"(weight {at})" in msg, msg
    if dim == 1:                                           # ti_adw_create is the same entry
        v = w.copy()
        v[3] = bad
        assert not _create(lib, H, L, 1, v, "f16x2", nd=False)
        assert "(weight 3)" in ti._lib.last_error()


def test_create_nd_checks_the_argument_list_before_the_weights(lib):
    """A wrong weight count is still reported as such: the weight scan runs over a validated array."""
    ti = pkg()
    w = np.full(10, np.inf)
    assert not _create(lib, 64, 3, 5, w, "f16x2")
    assert "weight count" in ti._lib.last_error()
