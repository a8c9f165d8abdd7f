"""Numpy restatement of the adw trainer (include/ti_hip.h ti_adw_train_*): FCNetMultiBeta forward and backward on the velocity loss,
clip_grad_norm_, Adam with L2 weight decay, the NaN skip, and the ReduceLROnPlateau scheduler of the training driver.  `dtype`
float64 is the reference arithmetic; float32 is the plain single-precision model the GPU bars are derived from (weights, inputs,
sums and SiLU in float32; the output gradient from the fp64 expression rounded once, as on the device).  Gradients come back as a
state dict and, through flat(), in the canonical layout.  Shared by tests/test_adw_train_host.py, tests/test_gpu_adw_train.py and
tests/golden/make_golden_adw_train.py."""
import numpy as np

import vloss_numpy as vn
from conftest import pkg


def spec(H, L, d):
    return pkg().weights.adw_param_spec(H, L, d, d)


def flat(sd, H, L, d):
    return pkg().weights.flatten_state_dict(sd, spec(H, L, d), dtype=np.float64)


def unflat(w, H, L, d):
    return pkg().weights.unflatten(np.asarray(w, np.float64), spec(H, L, d))


def _silu(z):
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-z))
    y = z * sg
    return y, sg + y * (1.0 - sg)


def _n_linear(sd, prefix):
    return sum(1 for k in sd if k.startswith(prefix + ".") and k.endswith(".weight"))


def _forward(sd, prefix, a, dtype):
    """-> (out, cache): cache[i] = (input of Linear i, silu' of its output or None)"""
    n = _n_linear(sd, prefix)
    h, cache = a.astype(dtype), []
    for i in range(n):
        W, b = sd[f"{prefix}.{2 * i}.weight"].astype(dtype), sd[f"{prefix}.{2 * i}.bias"].astype(dtype)
        z = h @ W.T + b
        if i == n - 1:
            cache.append((h, None))
            return z, cache
        y, dy = _silu(z)
        cache.append((h, dy))
        h = y
    raise AssertionError


def _backward(sd, prefix, cache, gz, dtype, grads):
    """gz: gradient at the output of the last Linear -> gradient at the MLP's input; weight and bias gradients into grads"""
    n = len(cache)
    for i in range(n - 1, -1, -1):
        h, _ = cache[i]
        grads[f"{prefix}.{2 * i}.weight"] = (gz.T @ h).astype(np.float64)
        grads[f"{prefix}.{2 * i}.bias"] = gz.sum(axis=0).astype(np.float64)
        ga = gz @ sd[f"{prefix}.{2 * i}.weight"].astype(dtype)
        if i == 0:
            return ga
        gz = ga * cache[i - 1][1]
    raise AssertionError


def loss_and_grad(sd, x0, x1, beta0, beta1, t, z=None, *, kind="standard", gamma="brownian", a=1.0, dtype=np.float64, round_states=True):
    """-> dict(loss [B] float64, mean, grads {key: float64 array}, b [halves, B, d]).  x0, x1 [B, d]; t [B]; z [B, d] (standard).
    round_states: the interpolated states are rounded to float32 once, as the device holds them (False: the reference's float64 run)."""
    x0, x1 = np.asarray(x0, np.float64).reshape(len(t), -1), np.asarray(x1, np.float64).reshape(len(t), -1)
    B, d = x0.shape
    two = kind == "standard"
    zz = None if z is None else np.asarray(z, np.float64).reshape(B, d)
    xt, _ = vn.interpolate(x0, x1, t, zz, kind=kind, gamma_kind=gamma, a=a, center="none")
    if round_states:
        xt = xt.astype(np.float32)
    halves = xt.shape[0]
    tt = np.asarray(t, np.float32)
    b0 = np.broadcast_to(np.asarray(beta0, np.float32).reshape(-1), (B,))
    b1 = np.broadcast_to(np.asarray(beta1, np.float32).reshape(-1), (B,))
    emb, ecache = _forward(sd, "beta_embed", np.stack([b0, b1, tt], 1), dtype)
    a0 = np.concatenate([xt.reshape(halves * B, d).astype(dtype), np.tile(tt[:, None].astype(dtype), (halves, 1)), np.tile(emb, (halves, 1))], 1)
    out, ncache = _forward(sd, "net", a0, dtype)
    bb = out.reshape(halves, B, d).astype(np.float64)
    l, _, _ = vn.loss(x0, x1, t, zz, bb[0], bb[1] if two else None, kind=kind, gamma_kind=gamma, a=a)
    dd = x1 - x0
    if two:
        gz = vn.gamma_dot(gamma, a, np.asarray(t, np.float64)[:, None]) * zz
        gout = np.concatenate([(bb[0] - (dd + gz)) / B, (bb[1] - (dd - gz)) / B], 0)
    else:
        gout = (bb[0] - dd) / B
    grads = {}
    ga0 = _backward(sd, "net", ncache, gout.astype(dtype), dtype, grads)
    ge = ga0[:B, d + 1] + ga0[B:, d + 1] if two else ga0[:, d + 1]
    _backward(sd, "beta_embed", ecache, ge[:, None].astype(dtype), dtype, grads)
    return dict(loss=l, mean=float(vn.fixed_order_sum(l) / B), grads=grads, b=bb)


def rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


def per_tensor_rel_l2(g, ref):
    """{key: rel-L2 of g[key] against ref[key]}"""
    return {k: rel_l2(g[k], ref[k]) for k in ref}


class Adam:
    """clip_grad_norm_(max_norm) then torch.optim.Adam(lr, betas, eps, weight_decay) on one flat fp64 vector, operation by operation as
    the header states them; step() returns True where the step was skipped (a non-finite entry, or a non-finite mean loss)."""

    def __init__(self, w, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=1.0):
        self.w = np.array(w, np.float64)
        self.m, self.v = np.zeros_like(self.w), np.zeros_like(self.w)
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_grad_norm
        self.n_applied = self.n_skipped = 0

    def step(self, g, mean=0.0):
        g = np.asarray(g, np.float64)
        ss = vn.fixed_order_sum(g * g)
        if not (np.isfinite(ss) and np.isfinite(mean)):
            self.n_skipped += 1
            return True
        coef = 1.0
        if self.max_norm > 0.0 and np.isfinite(self.max_norm):
            coef = min(1.0, self.max_norm / (np.sqrt(ss) + 1e-6))
        g = coef * g
        if self.wd != 0.0:
            g = g + self.wd * self.w
        k = self.n_applied + 1
        b1, b2 = self.betas
        self.m = b1 * self.m + (1.0 - b1) * g
        self.v = b2 * self.v + (1.0 - b2) * (g * g)
        step_size, bc2 = self.lr / (1.0 - b1 ** k), np.sqrt(1.0 - b2 ** k)
        self.w = self.w - step_size * (self.m / (np.sqrt(self.v) / bc2 + self.eps))
        self.n_applied = k
        return False


def adam_bound(w, lr, k):
    """16 k 2^-53 (|p| + lr): about 12 fp64 roundings per step, each at most one ulp of a quantity bounded by |p| or lr"""
    return 16.0 * k * 2.0 ** -53 * (np.abs(np.asarray(w, np.float64)) + lr)


class Plateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', threshold_mode='rel') on one learning rate"""

    def __init__(self, lr, factor=0.5, patience=10, threshold=1e-4, cooldown=0, min_lr=0.0, eps=1e-8):
        self.lr, self.factor, self.patience, self.threshold, self.cooldown, self.min_lr, self.eps = lr, factor, patience, threshold, cooldown, min_lr, eps
        self.best, self.num_bad, self.cooldown_counter = float("inf"), 0, 0

    def step(self, metric):
        metric = float(metric)
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.num_bad = metric, 0
        else:
            self.num_bad += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad = 0
        if self.num_bad > self.patience:
            new = max(self.lr * self.factor, self.min_lr)
            if self.lr - new > self.eps:
                self.lr = new
            self.cooldown_counter, self.num_bad = self.cooldown, 0
        return self.lr


def case(H, d, L, B, seed=0, per_row_beta=True):
    """Inputs of a gradient test: (state dict fp64, x0, x1 [B, d] float32, beta0, beta1 [B] float32, t [B] float32, z [B, d] float32).
    x0 ~ N(0, 1), x1 ~ N(4, 1.5^2): the target set is displaced against the base, as a target ensemble is, by more than the spread of
    x1 - x0 +- gamma' z.  The residual b - target of an untrained drift then has the same sign in almost every row, so a bias gradient
    -- a sum of such residuals over the rows -- is a sum of like terms.  With both sets centred the residuals have random signs, a
    scalar tensor such as beta_embed.4.bias is the small remainder of a random walk, and its RELATIVE error in any float32 evaluation
    is a matter of luck (measured: up to 2.2e-5 for the plain float32 model, against 1e-6 here).
    B = 1 is the row of the B = 17 inputs whose fp64 drift is largest: the loss bound is relative to the drift of the batch, and a single
    row at a zero crossing of the drift would leave it nothing to be relative to."""
    ti = pkg()
    sd = ti.synthetic.make_state_dict(spec(H, L, d), seed=1000 * H + 10 * d + L + seed, dtype=np.float64)
    n = 17 if B == 1 else B
    rs = np.random.RandomState(100 * H + 10 * d + L + B + seed)
    x0, x1, z = (rs.standard_normal((n, d)).astype(np.float32) for _ in range(3))
    x1 = (1.5 * x1 + 4.0).astype(np.float32)
    if per_row_beta:
        b0, b1 = rs.uniform(0.5, 1.5, n).astype(np.float32), rs.uniform(0.75, 2.0, n).astype(np.float32)
    else:
        b0, b1 = np.full(n, 1.0, np.float32), np.full(n, 1.25, np.float32)
    t = rs.uniform(0.05, 0.95, n).astype(np.float32)
    if B == 1:
        bb = loss_and_grad(sd, x0, x1, b0, b1, t, z, a=0.9)["b"]
        k = int(np.argmax(np.minimum(np.linalg.norm(bb[0], axis=1), np.linalg.norm(bb[1], axis=1))))
        x0, x1, z, b0, b1, t = (np.ascontiguousarray(v[k:k + 1]) for v in (x0, x1, z, b0, b1, t))
    return sd, x0, x1, b0, b1, t, z
