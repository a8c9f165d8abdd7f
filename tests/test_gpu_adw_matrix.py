"""GPU: every build of the FCNetMultiBeta (adw) drift kernels against the fp64 numpy restatement (adw_nd_numpy.py).

adw_mlp_kernel<NBK, SPLIT, TAN> (d = 1 and the beta embedding of every handle) and adw_mlp_nd_kernel<NBK, SPLIT, TAN, G> (2 <= d <= 16),
NBK = H / 16 for H in {32, 64, 128, 256}, SPLIT = f32 / f16x2, TAN = without / with the exact divergence: 32 builds.  What the cells of
adw_nd_numpy.MATRIX exercise (G = 8 / 4 / 2 / 1 tangent directions per pass at H = 32 / 64 / 128 / 256):
  * a short tangent group behind a full one (d = 9, 15 at G = 8; 5, 6, 13 at G = 4; 3, 15 at G = 2), full groups only, one short group;
  * the input padding: Kpad = d + 2 rounded up to 4 exact (d = 2, 6, 14) and with 1..3 zero columns, the b_out pad at every d mod 4;
  * depth: L = 1 (no hidden layer, an empty weight ring), the one-chunk ring (H = 32, L = 2) under two tangent groups, L = 9;
  * B = 209: three full workgroups and one of a full wave, a one-row wave and two empty waves; leading 1 / 16 / 17 / 64 / 65 rows alone;
    sentinels behind out[B * d] and out_div[B];
  * per-row and shared (beta0, beta1) (the dedupe table and U = B), a scalar time and per-row times;
  * Euler / Heun / per-trajectory dopri5 with dlogp at corners no fixture has;
  * |x| from 1e-6 to 1e6, the f16x2 activation domain (include/ti_hip.h ti_adw_create_nd) and input-layer tangent columns down to 1e-9.

Bars: drift and divergence rel-L2 <= 1e-5 against fp64 (tests/test_gpu_adw_nd.py); at the magnitude edges max(1e-5, 3 x the plain float32
model's own distance to fp64), the factor 3 for the kernels' summation order and v_exp / v_rcp against numpy's.  tests/test_adw_matrix_host.py
shows on the CPU that the float32 model alone stays 3x inside the bars at every cell.  `pytest -s` prints every figure and the worst per
(H, precision); the table of the last run is profiles/adw_matrix_parity.txt.  Needs a real MI355X: `pytest -m gpu`.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from adw_nd_numpy import (MATRIX, MATRIX_B, MATRIX_T, MODES, cell_inputs, cell_reference, cell_state_dict, drift as np_drift,
                          drift32, fixed_grid, mode_args)
from conftest import pkg, rel_l2
from oracle import ode

pytestmark = pytest.mark.gpu
F32 = np.float32
BAR = 1e-5                                     # tests/test_gpu_adw_nd.py:39-40
PRECISIONS = ["f32", "f16x2"]
F16_MAX = 65504.0
WORST = {}                                     # (H, precision) -> [drift rel-L2, cell, divergence rel-L2, cell]


class Cell:
    """The engine of one (H, d, L) cell; takes and returns [B, d] arrays at every d (the 1-D engine's own arrays are flat)."""

    def __init__(self, H, d, L, precision, sd=None):
        ti = pkg()
        self.H, self.d, self.L, self.precision = H, d, L, precision
        self.sd = cell_state_dict(H, L, d) if sd is None else sd
        spec = ti.weights.adw_param_spec(H, L, d, d)
        self.eng = ti.engine.AdwEngine(H, L, ti.weights.flatten_state_dict(self.sd, spec, dtype=np.float64), precision=precision, dim=d)

    def _x(self, x):
        return np.ascontiguousarray(x[:, 0] if self.d == 1 else x, F32)

    def drift(self, x, t, b0, b1, return_div=False):
        r = self.eng.drift(self._x(x), t, b0, b1, return_div=return_div)
        return (r[0].reshape(x.shape), r[1]) if return_div else r.reshape(x.shape)

    def rollout(self, x, b0, b1, grid, **kw):
        r = self.eng.rollout(self._x(x), b0, b1, grid, **kw)
        return (r[0].reshape((-1,) + x.shape),) + tuple(r[1:])

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module", autouse=True)
def worst_error_table():
    yield
    if WORST:
        print("\nadw matrix: worst rel-L2 against fp64 per (H, precision) over the cells of adw_nd_numpy.MATRIX, B = %d, bar %.0e" % (MATRIX_B, BAR))
        for (H, prec), (eb, cb, ed, cd) in sorted(WORST.items()):
            print(f"adw matrix: H {H:3d} {prec:5s}  drift {eb:.2e} at (d, L, mode) = {cb}   divergence {ed:.2e} at {cd}")


# ------------------------------------------------------------------------------------------------ 1. the matrix
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,d,L", MATRIX)
def test_cell_drift_and_divergence_vs_fp64(H, d, L, precision):
    inp, c = cell_inputs(d), Cell(H, d, L, precision)
    w = WORST.setdefault((H, precision), [0.0, None, 0.0, None])
    for mode in MODES:
        t, b0, b1 = mode_args(inp, mode)
        rb, rd = cell_reference(H, d, L, mode)
        b, div = c.drift(inp.x, t, b0, b1, return_div=True)
        assert b.shape == (MATRIX_B, d) and div.shape == (MATRIX_B,)
        eb, ed = rel_l2(b, rb), rel_l2(div, rd)
        print(f"\n  H {H} d {d} L {L} {precision} t {mode[0]} beta {mode[1]}: drift {eb:.2e} divergence {ed:.2e}", end="")
        if eb > w[0]:
            w[0], w[1] = eb, (d, L, "/".join(mode))
        if ed > w[2]:
            w[2], w[3] = ed, (d, L, "/".join(mode))
        assert np.isfinite(b).all() and np.isfinite(div).all(), mode
        assert eb <= BAR, (mode, eb)
        assert ed <= BAR, (mode, ed)
        np.testing.assert_array_equal(c.drift(inp.x, t, b0, b1), b)                    # the drift-only build: the same primal bits
        if mode[0] == "scalar":                                                        # one time == that time in every row
            tb, td = c.drift(inp.x, np.full(MATRIX_B, MATRIX_T, F32), b0, b1, return_div=True)
            np.testing.assert_array_equal(tb, b)
            np.testing.assert_array_equal(td, div)
    c.close()


# ------------------------------------------------------------------------------------------------ 2. batch edges
EDGE_CELLS = [(32, 9, 2), (256, 3, 5), (128, 1, 4)]          # nd kernel with two tangent groups, nd kernel with G = 1, the 1-D kernel
EDGE_ROWS = [1, 16, 17, 64, 65]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,d,L", EDGE_CELLS)
def test_leading_rows_alone_equal_their_rows_of_the_full_batch(H, d, L, precision):
    inp, c = cell_inputs(d), Cell(H, d, L, precision)
    for mode in (("scalar", "rows"), ("rows", "rows"), ("scalar", "one")):
        t, b0, b1 = mode_args(inp, mode)
        fb, fd = c.drift(inp.x, t, b0, b1, return_div=True)
        assert np.isfinite(fb).all() and np.isfinite(fd).all()
        for n in EDGE_ROWS:
            tn = t if mode[0] == "scalar" else t[:n]
            b, div = c.drift(inp.x[:n], tn, b0[:n], b1[:n], return_div=True)
            np.testing.assert_array_equal(b, fb[:n], err_msg=str((mode, n)))
            np.testing.assert_array_equal(div, fd[:n], err_msg=str((mode, n)))
            np.testing.assert_array_equal(c.drift(inp.x[:n], tn, b0[:n], b1[:n]), fb[:n], err_msg=str((mode, n)))
    c.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,d,L", EDGE_CELLS)
def test_rows_past_B_are_never_stored(H, d, L, precision):
    """Rows past B are clamped to row B - 1 for their loads and must not be stored: the outputs sit in front of 64 rows of sentinel
    inside the same allocation, and every sentinel survives.  (Nothing here reaches outside an allocation.)"""
    torch = pytest.importorskip("torch")
    ti = pkg()
    lib, mem = ti._lib.lib(), ti._lib.MEM_DEVICE
    inp, c = cell_inputs(d), Cell(H, d, L, precision)
    sentinel = F32(-12345.678)
    dev = lambda a: torch.from_numpy(np.array(a, F32)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for n in EDGE_ROWS + [MATRIX_B]:
        x, b0, b1, tv = dev(inp.x[:n]), dev(inp.b0[:n]), dev(inp.b1[:n]), dev(inp.tv[:n])
        for per_row in (False, True):
            out = torch.full((n * d + 64 * d,), float(sentinel), dtype=torch.float32, device="cuda")
            div = torch.full((n + 64,), float(sentinel), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            if per_row:
                ti._lib.check(lib.ti_adw_drift_tv(c.eng.h, ptr(x), ptr(tv), ptr(b0), ptr(b1), n, ptr(out), ptr(div), mem))
            else:
                ti._lib.check(lib.ti_adw_drift_div(c.eng.h, ptr(x), MATRIX_T, ptr(b0), ptr(b1), n, ptr(out), ptr(div), mem))
            o, dv = out.cpu().numpy(), div.cpu().numpy()
            assert (o[n * d:] == sentinel).all() and (dv[n:] == sentinel).all(), (n, per_row)
            hb, hd = c.drift(inp.x[:n], inp.tv[:n] if per_row else MATRIX_T, inp.b0[:n], inp.b1[:n], return_div=True)
            np.testing.assert_array_equal(o[:n * d].reshape(n, d), hb)
            np.testing.assert_array_equal(dv[:n], hd)
    c.close()


# ------------------------------------------------------------------------------------------------ 3. rollouts at uncovered corners
ROLL_CELLS = [(32, 9, 2), (64, 5, 1), (128, 3, 4)]           # every one with a short tangent group behind a full one
ROLL_B = 70                                                  # one full workgroup and six rows
TRAJ_ODE_ROWS = (0, 15, 16, 17, 63, 64, 65, 69)              # the attempt counts are replayed on the CPU for the rows at wave / workgroup seams


@functools.lru_cache(maxsize=None)
def _fixed_grid_reference(H, d, L, scheme):
    inp = cell_inputs(d, ROLL_B)
    return fixed_grid(cell_state_dict(H, L, d), inp.x, inp.b0, inp.b1, pkg().engine.time_grid(0.0, 1.0, 6), scheme)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,d,L", ROLL_CELLS)
def test_euler_heun_with_dlogp_vs_fp64_fixed_grid(H, d, L, precision):
    inp, c = cell_inputs(d, ROLL_B), Cell(H, d, L, precision)
    grid = pkg().engine.time_grid(0.0, 1.0, 6)
    for scheme in ("euler", "heun"):
        path, dl, nfe = c.rollout(inp.x, inp.b0, inp.b1, grid, scheme=scheme, return_dlogp=True)
        rp, rdl = _fixed_grid_reference(H, d, L, scheme)
        assert path.shape == rp.shape and dl.shape == rdl.shape and nfe == 5 * (2 if scheme == "heun" else 1)
        ep, ed = rel_l2(path, rp), rel_l2(dl[1:], rdl[1:])
        print(f"\n  H {H} d {d} L {L} {precision} {scheme}: path {ep:.2e} dlogp {ed:.2e}", end="")
        assert ep <= 1e-5, (scheme, ep)                        # tests/test_gpu_adw_nd.py:52
        assert ed <= 1e-5, (scheme, ed)                        # tests/test_gpu_adw_nd.py:56
        np.testing.assert_array_equal(c.rollout(inp.x, inp.b0, inp.b1, grid, scheme=scheme)[0], path)
    c.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,d,L", ROLL_CELLS)
def test_dopri5_trajectory_rows_equal_themselves_alone(H, d, L, precision):
    inp, c = cell_inputs(d, ROLL_B), Cell(H, d, L, precision)
    grid = np.linspace(0, 1, 4).astype(F32)
    kw = dict(scheme="dopri5", step_control="trajectory", return_dlogp=True, rtol=1e-5, atol=1e-5)
    path, dl, _ = c.rollout(inp.x, inp.b0, inp.b1, grid, **kw)
    acc, rej = c.eng.step_counts(ROLL_B)
    assert np.isfinite(path).all() and np.isfinite(dl).all()
    for b in range(ROLL_B):
        sb0, sb1 = inp.b0[b:b + 1], inp.b1[b:b + 1]
        ap, adl, _ = c.rollout(inp.x[b:b + 1], sb0, sb1, grid, **kw)
        np.testing.assert_array_equal(ap[:, 0], path[:, b], err_msg=str(b))
        np.testing.assert_array_equal(adl[:, 0], dl[:, b], err_msg=str(b))
        a1, r1 = c.eng.step_counts(1)
        assert (a1[0], r1[0]) == (acc[b], rej[b]), b
        if b not in TRAJ_ODE_ROWS:
            continue

        def own(t, y):
            o, div = c.drift(np.ascontiguousarray(y[0], F32), t, sb0, sb1, return_div=True)
            return [o, (-div * F32(1e-2)).astype(F32)]

        sol, nfe = ode.odeint(own, [inp.x[b:b + 1], np.zeros(1, F32)], grid, "dopri5", 1e-5, 1e-5)
        assert acc[b] + rej[b] == (nfe - 2) // 6, b
        assert np.abs(path[-1, b] - sol[0][-1, 0]).max() <= 1e-5 * max(1.0, np.abs(sol[0][-1]).max()), b
    c.close()


# ------------------------------------------------------------------------------------------------ 4. magnitude edges
MAG_CELLS = [(64, 3, 3), (256, 5, 5)]
MAG_B = 48
MAG_MODE = ("scalar", "rows")


def _bars(sd, x, t, b0, b1, rb, rd):
    """max(1e-5, 3 x the float32 model's distance to fp64) for the drift and the divergence."""
    b32, d32 = drift32(sd, x, t, b0, b1, return_div=True)
    return max(BAR, 3 * rel_l2(b32, rb)), max(BAR, 3 * rel_l2(d32, rd))


@functools.lru_cache(maxsize=None)
def _scaled_case(H, d, L, scale):
    """x ~ N(0, 1) * scale: (x, t, b0, b1, fp64 drift, fp64 divergence, peak |activation| per row, drift bar, divergence bar)."""
    inp, sd = cell_inputs(d, MAG_B, False), cell_state_dict(H, L, d)
    t, b0, b1 = mode_args(inp, MAG_MODE)
    x = inp.x * F32(scale)
    rb, rd, peak = np_drift(sd, x, t, b0, b1, return_div=True, return_peak=True)
    return (x, t, b0, b1, rb, rd, peak) + _bars(sd, x, t, b0, b1, rb, rd)


@pytest.mark.parametrize("precision,scale", [(p, s) for p in PRECISIONS for s in (1e-6, 1e-3, 1e2, 1e3, 1e4)] + [("f32", 1e5), ("f32", 1e6)])
@pytest.mark.parametrize("H,d,L", MAG_CELLS)
def test_input_magnitudes(H, d, L, precision, scale):
    x, t, b0, b1, rb, rd, peak, bar_b, bar_d = _scaled_case(H, d, L, scale)
    if precision == "f16x2":
        assert peak.max() < F16_MAX / 2                      # inside the documented domain of the split-fp16 operands
    c = Cell(H, d, L, precision)
    b, div = c.drift(x, t, b0, b1, return_div=True)
    eb, ed = rel_l2(b, rb), rel_l2(div, rd)
    print(f"\n  H {H} d {d} L {L} {precision} x * {scale:g}: drift {eb:.2e} (bar {bar_b:.1e}) divergence {ed:.2e} (bar {bar_d:.1e}) "
          f"peak activation {peak.max():.3g}", end="")
    assert np.isfinite(b).all() and np.isfinite(div).all()
    assert eb <= bar_b, (eb, bar_b)
    assert ed <= bar_d, (ed, bar_d)
    c.close()


DOMAIN_IN, DOMAIN_OUT = 1e3, 1e7                             # row scales: every third row is pushed out of the fp16 range


@functools.lru_cache(maxsize=None)
def _domain_case(H, d, L):
    inp, sd = cell_inputs(d, MAG_B, False), cell_state_dict(H, L, d)
    t, b0, b1 = mode_args(inp, MAG_MODE)
    x = (inp.x * np.where(np.arange(MAG_B) % 3 == 2, DOMAIN_OUT, DOMAIN_IN)[:, None]).astype(F32)
    rb, rd, peak = np_drift(sd, x, t, b0, b1, return_div=True, return_peak=True)
    return x, t, b0, b1, rb, rd, peak


@pytest.mark.parametrize("H,d,L", MAG_CELLS)
def test_f16x2_activation_domain(H, d, L):
    """include/ti_hip.h ti_adw_create_nd: f16x2 holds the f32 path's parity while every hidden activation stays below 65504; a row
    beyond it comes back non-finite (never finite and wrong), leaves the other rows' bits alone, and makes a rollout report TI_E_NAN."""
    ti = pkg()
    x, t, b0, b1, rb, rd, peak = _domain_case(H, d, L)
    inside, outside = peak < F16_MAX / 2, peak > 2 * F16_MAX
    assert (inside | outside).all() and inside.sum() >= MAG_B // 2 and outside.sum() >= MAG_B // 4
    sd = cell_state_dict(H, L, d)
    c = Cell(H, d, L, "f16x2")
    b, div = c.drift(x, t, b0, b1, return_div=True)
    bar_b, bar_d = _bars(sd, x[inside], t, b0[inside], b1[inside], rb[inside], rd[inside])
    eb, ed = rel_l2(b[inside], rb[inside]), rel_l2(div[inside], rd[inside])
    print(f"\n  H {H} d {d} L {L} f16x2 domain: in-range rows drift {eb:.2e} divergence {ed:.2e}; "
          f"{int((~np.isfinite(b).all(axis=1) | ~np.isfinite(div))[outside].sum())} of {int(outside.sum())} out-of-range rows non-finite", end="")
    assert np.isfinite(b[inside]).all() and np.isfinite(div[inside]).all()
    assert eb <= bar_b and ed <= bar_d, (eb, bar_b, ed, bar_d)
    ab, adiv = c.drift(x[inside], t, b0[inside], b1[inside], return_div=True)
    np.testing.assert_array_equal(ab, b[inside])
    np.testing.assert_array_equal(adiv, div[inside])
    for r in np.flatnonzero(outside):
        if np.isfinite(b[r]).all() and np.isfinite(div[r]):
            s = slice(r, r + 1)
            rbar_b, rbar_d = _bars(sd, x[s], t, b0[s], b1[s], rb[s], rd[s])
            assert rel_l2(b[s], rb[s]) <= rbar_b and rel_l2(div[s], rd[s]) <= rbar_d, ("finite and wrong", r, b[r], rb[r], div[r], rd[r])
    grid = np.linspace(0, 1, 3).astype(F32)
    with pytest.raises(ti._lib.TiError) as e:
        c.rollout(x, b0, b1, grid, scheme="euler")
    assert e.value.code == ti._lib.TI_E_NAN
    path, _ = c.rollout(x[inside], b0[inside], b1[inside], grid, scheme="euler")     # the in-range rows alone roll out
    assert np.isfinite(path).all()
    c.close()


@functools.lru_cache(maxsize=None)
def _small_tangent_case(H, d, L, k):
    inp, sd = cell_inputs(d, MAG_B, False), dict(cell_state_dict(H, L, d))
    w = sd["net.0.weight"].copy()
    w[:, :d] *= k
    sd["net.0.weight"] = w
    t, b0, b1 = mode_args(inp, MAG_MODE)
    rb, rd = np_drift(sd, inp.x, t, b0, b1, return_div=True)
    return (sd, inp.x, t, b0, b1, rb, rd) + _bars(sd, inp.x, t, b0, b1, rb, rd)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [1e-3, 1e-6, 1e-9])
@pytest.mark.parametrize("H,d,L", MAG_CELLS)
def test_small_tangents(H, d, L, k, precision):
    """x-columns of net.0.weight scaled by k: the tangent rows start at k.  The divergence is held to the absolute form the dlogp integral
    cares about; its relative error is asserted for f32 and printed for f16x2, whose unscaled tangent operands fall into fp16 subnormals
    (DESIGN.md 3.2)."""
    sd, x, t, b0, b1, rb, rd, bar_b, bar_d = _small_tangent_case(H, d, L, k)
    c = Cell(H, d, L, precision, sd)
    b, div = c.drift(x, t, b0, b1, return_div=True)
    eb, ed = rel_l2(b, rb), rel_l2(div, rd)
    print(f"\n  H {H} d {d} L {L} {precision} tangent columns * {k:g}: drift {eb:.2e} divergence rel {ed:.2e} "
          f"max |err| {np.abs(div - rd).max():.2e} at |div| <= {np.abs(rd).max():.2e}", end="")
    assert np.isfinite(b).all() and np.isfinite(div).all()
    assert eb <= bar_b, (eb, bar_b)
    assert (np.abs(div - rd) <= 1e-5 * (np.abs(rd) + 1.0)).all(), np.abs(div - rd).max()
    if precision == "f32":
        assert ed <= bar_d, (ed, bar_d)
    c.close()
