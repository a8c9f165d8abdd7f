"""fp64 numpy restatement of FCNetMultiBeta(d, d, H, L) (the reference's adw/thermo/models/simple.py) and of its exact divergence
by forward-mode differentiation, one tangent direction per input coordinate.  Used by the d-dimensional adw tests: it pins the
fixture layout (tests/golden/make_golden_nd.py) on the CPU, and serves as the fp64 drift of the GPU dopri5 comparison."""
import numpy as np

from conftest import GOLDEN, pkg

CASES = ["adw_nd2_h64", "adw_nd3_h256", "adw_nd16_h128", "adw_nd2_ctor_h32"]


def _silu(z):
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


def _mlp(sd, prefix, a, tangent_cols=None):
    """a [B, K] through Linear, SiLU, ..., Linear; with tangent_cols = number of leading input columns to differentiate,
    also returns the forward-mode tangents' output trace sum_i d out_i / d a_i."""
    n = n_linear(sd, prefix)
    h, T = a, None
    for i in range(n):
        Wt, b = sd[f"{prefix}.{2 * i}.weight"], sd[f"{prefix}.{2 * i}.bias"]
        z = h @ Wt.T + b
        if tangent_cols is not None:
            T = Wt[None, :, :tangent_cols].repeat(a.shape[0], 0) if T is None else np.einsum("ok,bkd->bod", Wt, T)
        if i == n - 1:
            h = z
            break
        h, dy = _silu(z)
        if T is not None:
            T = dy[:, :, None] * T
    if tangent_cols is None:
        return h
    return h, np.einsum("bii->b", T)


def drift(sd, x, t, beta0, beta1, return_div=False):
    """b(x, t) [B, d] in fp64; t a scalar or [B]; with return_div also sum_i d b_i / d x_i [B] (no 1e-2 factor)."""
    x = np.asarray(x, np.float64)
    B, d = x.shape
    t = np.broadcast_to(np.asarray(t, np.float64).reshape(-1), (B,))
    b0 = np.broadcast_to(np.asarray(beta0, np.float64).reshape(-1), (B,))
    b1 = np.broadcast_to(np.asarray(beta1, np.float64).reshape(-1), (B,))
    emb = _mlp(sd, "beta_embed", np.stack([b0, b1, t], 1))
    a = np.concatenate([x, t[:, None], emb], 1)
    if not return_div:
        return _mlp(sd, "net", a)
    return _mlp(sd, "net", a, tangent_cols=d)
