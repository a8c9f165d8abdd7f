"""fp64 numpy restatement of FCNetMultiBeta(d, d, H, L) (the reference's adw/thermo/models/simple.py) and of its exact divergence
by forward-mode differentiation, one tangent direction per input coordinate.  Used by the d-dimensional adw tests: it pins the
fixture layout (tests/golden/make_golden_nd.py) on the CPU, and serves as the fp64 drift of the GPU dopri5 comparison.  d = 1 (x [B, 1])
and L = 1 are handled; adw_param_spec(H, L, 1, 1) is the 1-D spec.  drift32 is the same network in plain float32 (the yardstick the bars
of the instantiation matrix are derived from); MATRIX and the cell_* helpers are the shared inputs and references of
tests/test_adw_matrix_host.py and tests/test_gpu_adw_matrix.py."""
import functools
import types

import numpy as np

from conftest import GOLDEN, pkg

CASES = ["adw_nd2_h64", "adw_nd3_h256", "adw_nd16_h128", "adw_nd2_ctor_h32"]


def _silu(z):
    with np.errstate(over="ignore"):             # exp(-z) of a large negative z is inf and 1 / inf = 0, as on the device
        sg = 1.0 / (1.0 + np.exp(-z))
    y = z * sg
    return y, sg + y * (1.0 - sg)


def load_case(name):
    """(fixture dict, state_dict of fp64 arrays); synthetic weights are regenerated from the stored seed."""
    import os
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    sd = {k[4:]: v for k, v in g.items() if k.startswith("sd::")}
    if not sd:
        ti = pkg()
        d, H, L = int(g["dim"]), int(g["hidden"]), int(g["num_layers"])
        sd = ti.synthetic.make_state_dict(ti.weights.adw_param_spec(H, L, d, d), seed=int(g["seed"]), dtype=np.float64)
    return g, sd


def n_linear(sd, prefix):
    return sum(1 for k in sd if k.startswith(prefix + ".") and k.endswith(".weight"))


def _mlp(sd, prefix, a, tangent_cols=None, dtype=np.float64, peak=None):
    """a [B, K] through Linear, SiLU, ..., Linear in `dtype`; with tangent_cols = number of leading input columns to differentiate,
    also returns the forward-mode tangents' output trace sum_i d out_i / d a_i.  peak [B]: raised in place to each row's largest
    |SiLU output| of this MLP."""
    n = n_linear(sd, prefix)
    h, T = a.astype(dtype), None
    for i in range(n):
        Wt, b = sd[f"{prefix}.{2 * i}.weight"].astype(dtype), sd[f"{prefix}.{2 * i}.bias"].astype(dtype)
        z = h @ Wt.T + b
        if tangent_cols is not None:
            T = Wt[None, :, :tangent_cols].repeat(a.shape[0], 0) if T is None else np.matmul(Wt, T)
        if i == n - 1:
            h = z
            break
        h, dy = _silu(z)
        if peak is not None:
            np.maximum(peak, np.abs(h).max(axis=1), out=peak)
        if T is not None:
            T = dy[:, :, None] * T
    if tangent_cols is None:
        return h
    return h, np.einsum("bii->b", T)


def _drift(sd, x, t, beta0, beta1, return_div, dtype, return_peak=False):
    x = np.asarray(x, dtype)
    B, d = x.shape
    t = np.broadcast_to(np.asarray(t, dtype).reshape(-1), (B,))
    b0 = np.broadcast_to(np.asarray(beta0, dtype).reshape(-1), (B,))
    b1 = np.broadcast_to(np.asarray(beta1, dtype).reshape(-1), (B,))
    peak = np.zeros(B, np.float64) if return_peak else None
    emb = _mlp(sd, "beta_embed", np.stack([b0, b1, t], 1), dtype=dtype, peak=peak)
    a = np.concatenate([x, t[:, None], emb], 1)
    res = _mlp(sd, "net", a, tangent_cols=d if return_div else None, dtype=dtype, peak=peak)
    res = tuple(res) if return_div else (res,)
    if return_peak:
        res += (peak,)
    return res if len(res) > 1 else res[0]


def drift(sd, x, t, beta0, beta1, return_div=False, return_peak=False):
    """b(x, t) [B, d] in fp64; t a scalar or [B]; with return_div also sum_i d b_i / d x_i [B] (no 1e-2 factor); with return_peak
    also each row's largest |SiLU output| over both MLPs [B] (what a split-fp16 operand of the kernels has to hold)."""
    return _drift(sd, x, t, beta0, beta1, return_div, np.float64, return_peak)


def drift32(sd, x, t, beta0, beta1, return_div=False):
    """The same network in plain numpy float32 (weights, inputs, sums and SiLU; no fp16 anywhere): the distance of honest fp32
    arithmetic to drift(), from which the bars of the matrix tests are derived."""
    return _drift(sd, x, t, beta0, beta1, return_div, np.float32)


def fixed_grid(sd, x, beta0, beta1, grid, scheme):
    """(path [n, B, d], dlogp [n, B] (* 1e2 like the reference)) of Euler / Heun steps over drift() in fp64; the step sizes are the
    fp32 differences of the fp32 grid, as the engine takes them."""
    xs, dl = np.asarray(x, np.float64), np.zeros(len(x))
    path, dls = [xs], [dl]
    for k in range(len(grid) - 1):
        dt = np.float64(np.float32(grid[k + 1]) - np.float32(grid[k]))
        b1_, d1 = drift(sd, xs, np.float32(grid[k]), beta0, beta1, return_div=True)
        if scheme == "euler":
            xs, dl = xs + dt * b1_, dl - dt * d1 * 1e-2
        else:
            b2_, d2 = drift(sd, xs + dt * b1_, np.float32(grid[k + 1]), beta0, beta1, return_div=True)
            xs, dl = xs + 0.5 * dt * (b1_ + b2_), dl - 0.5 * dt * (d1 + d2) * 1e-2
        path.append(xs); dls.append(dl)
    return np.stack(path), np.stack(dls) * 1e2


# ------------------------------------------------------------------------------------------------ the instantiation matrix
# (H, d, L) cells of tests/test_adw_matrix_host.py and tests/test_gpu_adw_matrix.py.  The tangent group of adw_mlp_nd_kernel is
# G = 8 / 4 / 2 / 1 at H = 32 / 64 / 128 / 256: every width has d = 1 (adw_mlp_kernel), one short group, full groups only, and a short
# group behind a full one (d = 9, 15 at G = 8; 5, 6, 13 at G = 4; 3, 15 at G = 2); Kpad = d + 2 rounded up to 4 is exact at d = 2, 6, 14;
# L = 1 has no hidden layer, (32, ., 2) is the one-chunk weight ring.
MATRIX = ([(32, d, L) for d in (1, 7, 8, 9, 15, 16) for L in (1, 2, 3)] + [(64, d, L) for d in (1, 3, 4, 5, 6, 13) for L in (1, 3)] +
          [(128, d, L) for d in (1, 2, 3, 14, 15) for L in (1, 4)] + [(256, d, L) for d in (1, 2, 7, 16) for L in (1, 5)] +
          [(32, 9, 9), (256, 3, 9)])
MATRIX_B = 209          # three full workgroups of 64 rows, then one with a full wave, a one-row wave and two empty waves
MATRIX_T = 0.37
MODES = [(tk, bk) for bk in ("rows", "one") for tk in ("scalar", "rows")]        # (time per call / per row, (beta0, beta1) per row / one pair)
TAN_GROUP = {32: 8, 64: 4, 128: 2, 256: 1}


def cell_state_dict(H, L, d, seed=None):
    ti = pkg()
    return ti.synthetic.make_state_dict(ti.weights.adw_param_spec(H, L, d, d), seed=1000 * H + 10 * d + L if seed is None else seed,
                                        dtype=np.float64)


@functools.lru_cache(maxsize=None)
def cell_inputs(d, B=MATRIX_B, row_scale=True):
    """x [B, d] ~ N(0, 1), row r scaled by linspace(0.3, 3, B)[r]; one (beta0, beta1) and one time per row.  float32, read-only."""
    rs = np.random.RandomState(7000 + d)
    x = rs.standard_normal((B, d))
    if row_scale:
        x = x * np.linspace(0.3, 3.0, B)[:, None]
    out = types.SimpleNamespace(x=x.astype(np.float32), b0=rs.uniform(0.5, 1.5, B).astype(np.float32),
                                b1=rs.uniform(0.75, 2.0, B).astype(np.float32), tv=rs.uniform(0.0, 1.0, B).astype(np.float32))
    for a in vars(out).values():
        a.setflags(write=False)
    return out


def mode_args(inp, mode):
    """(t, beta0, beta1) of a MODES entry over cell_inputs."""
    tk, bk = mode
    B = inp.x.shape[0]
    b0, b1 = (inp.b0, inp.b1) if bk == "rows" else (np.full(B, 1.0, np.float32), np.full(B, 1.25, np.float32))
    return (MATRIX_T if tk == "scalar" else inp.tv), b0, b1


@functools.lru_cache(maxsize=None)
def cell_reference(H, d, L, mode, fp32=False):
    """(drift [B, d], divergence [B]) of a matrix cell in fp64 (fp32: the plain float32 model), computed once and shared."""
    inp = cell_inputs(d)
    t, b0, b1 = mode_args(inp, mode)
    out = (drift32 if fp32 else drift)(cell_state_dict(H, L, d), inp.x, t, b0, b1, return_div=True)
    for a in out:
        a.setflags(write=False)
    return out
