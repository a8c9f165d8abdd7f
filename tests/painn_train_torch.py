"""A torch restatement of the cPaiNN forward pass (SURVEY.md section 8a, rows K1 .. K9) and of the velocity loss on it, for the three
variants and any edge template, in float64 or float32.  Its autograd is the yardstick of the molecule trainer (ti_painn_train_*) at
any shape: tests/test_painn_train_host.py pins it against the reference's own gradients, tests/test_gpu_painn_train.py compares the
device gradients with it.  Parameters are a dict of tensors under the reference's state_dict keys (weights.painn_param_spec)."""
import math

import numpy as np
import torch

N_COND = {0: 2, 1: 1, 2: 0}
COMBINE_IDX = {0: 7, 1: 6, 2: 5}
DEFAULTS = dict(temp_length=10.0, time_length=10.0, length_scale=10.0, temp_mean=650.0, temp_range=700.0)


def posenc(x, length, F):
    """PositionalEncoder: [cos(x / length k pi), sin(x / length k pi)] interleaved, k = 1 .. F / 2; x [...] -> [..., F]"""
    k = torch.arange(1, F // 2 + 1, dtype=x.dtype)
    arg = (x / length)[..., None] * k * math.pi
    return torch.stack([torch.cos(arg), torch.sin(arg)], dim=-1).reshape(*x.shape, F)


def mlp(P, prefix, x):
    """Linear, LayerNorm (eps 1e-5, biased variance), SiLU, twice over, then a last Linear"""
    F_ = torch.nn.functional
    for a, b in (("0", "1"), ("3", "4")):
        x = F_.linear(x, P[f"{prefix}.{a}.weight"], P[f"{prefix}.{a}.bias"])
        x = F_.silu(F_.layer_norm(x, x.shape[-1:], P[f"{prefix}.{b}.weight"], P[f"{prefix}.{b}.bias"], 1e-5))
    return F_.linear(x, P[f"{prefix}.6.weight"], P[f"{prefix}.6.bias"])


def forward(P, variant, F, L, src, dst, etype, atom_ids, x, t, cond, **kw):
    """x [R, A, 3], t [R], cond [R, A, ncond] | None -> the drift [R, A, 3].  src, dst, etype: the molecule's edge template."""
    c = dict(DEFAULTS); c.update(kw)
    R, A = x.shape[0], x.shape[1]
    dt = x.dtype
    src, dst, etype, atom_ids = (torch.as_tensor(np.asarray(a), dtype=torch.long) for a in (src, dst, etype, atom_ids))
    ci = COMBINE_IDX[variant]
    base = f"net.{ci + 1}.layers"
    r = x[:, src] - x[:, dst]                                                   # [R, E, 3]
    d = r.norm(dim=-1)
    edir = r / (1.0 + d)[..., None]
    enc = posenc(d, c["length_scale"], F)
    e = P["net.2.embedding.weight"][etype][None].expand(R, -1, -1)
    parts = [P["net.3.embedding.weight"][atom_ids][None].expand(R, -1, -1)]
    for k in range(N_COND[variant]):
        parts.append(posenc((cond[..., k] - c["temp_mean"]) / c["temp_range"], c["temp_length"], F))
    parts.append(posenc(t[:, None].expand(R, A), c["time_length"], F))
    s = mlp(P, f"net.{ci}.mlp.mlp", torch.cat(parts, dim=-1))
    v = torch.zeros(R, A, F, 3, dtype=dt)
    for l in range(L):
        h = mlp(P, f"{base}.{2 * l}.phi.mlp", torch.cat([s[:, src], e], dim=-1)) * mlp(P, f"{base}.{2 * l}.w.mlp", enc)
        gates, scale, ds, de, cross = torch.split(h, F, dim=-1)
        ed3 = edir[:, :, None, :].expand(-1, -1, F, -1)
        dv = scale[..., None] * ed3 + gates[..., None] * v[:, src] + cross[..., None] * torch.cross(ed3, v[:, dst], dim=-1)
        v = v + torch.zeros_like(v).index_add(1, dst, dv)
        s = s + torch.zeros_like(s).index_add(1, dst, ds)
        e = e + de
        U, V = P[f"{base}.{2 * l + 1}.u.linear.weight"], P[f"{base}.{2 * l + 1}.v.linear.weight"]
        uv = torch.einsum("gf,rafc->ragc", U, v)
        vv = torch.einsum("gf,rafc->ragc", V, v)
        n = vv.norm(dim=-1)
        g, q, a = torch.split(mlp(P, f"{base}.{2 * l + 1}.mlp.mlp", torch.cat([n, s], dim=-1)), F, dim=-1)
        v = v + uv * g[..., None]
        s = s + n * n * q + a
    ro = mlp(P, f"{base}.{2 * L}.mlp.mlp", s)
    Vv = torch.einsum("gf,rafc->ragc", P[f"{base}.{2 * L}.V.linear.weight"], v)[:, :, 0]      # [R, A, 3]
    return Vv * ro[..., 1:2]


def gamma_dot(kind, a, t):
    if kind == "brownian":
        return a * (1.0 - 2.0 * t) / (2.0 * torch.sqrt(a * t * (1.0 - t)))
    if kind == "sin2":
        return 2.0 * math.pi * torch.sin(math.pi * t) * torch.cos(math.pi * t)
    sp, sm = torch.sigmoid(a * (t - 0.5) + 1.0), torch.sigmoid(a * (t - 0.5) - 1.0)
    return float(np.float32(2.2)) * a * ((1.0 - sp) * sp - (1.0 - sm) * sm)


def loss_rows(P, model, xt, x0, x1, t, z, cond, kind="standard", gamma="brownian", a=1.0):
    """The loss rows l_b [B] on given states xt [halves, B, A, 3] (the velocity-loss block of include/ti_hip.h): 1/2 |b|^2 - target . b
    summed over the molecule's entries and both halves; the mean of the trainer is sum(l_b) / (B A).  model: dict(variant, F, L, src,
    dst, etype, atom_ids, and encoder lengths)."""
    halves, B = xt.shape[0], xt.shape[1]
    tt = t.repeat(halves)
    cc = None if cond is None else cond.repeat(halves, 1, 1)
    b = forward(P, x=xt.reshape(halves * B, *xt.shape[2:]), t=tt, cond=cc, **model).reshape(xt.shape)
    dlt = x1 - x0
    if kind == "one_sided":
        return (0.5 * b[0] * b[0] - dlt * b[0]).sum(dim=(1, 2))
    gz = gamma_dot(gamma, a, t)[:, None, None] * z
    return (0.5 * b[0] * b[0] - (dlt + gz) * b[0] + 0.5 * b[1] * b[1] - (dlt - gz) * b[1]).sum(dim=(1, 2))


def grads(flat, spec, model, xt, x0, x1, t, z, cond, dtype=torch.float64, **lk):
    """-> (loss rows [B], mean, {key: gradient of the mean}) with every input cast to `dtype`."""
    P, o = {}, 0
    for k, shape in spec:
        n = int(np.prod(shape))
        P[k] = torch.tensor(np.asarray(flat[o:o + n], np.float64).reshape(shape), dtype=dtype, requires_grad=True)
        o += n
    cv = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype)
    rows = loss_rows(P, model, cv(xt), cv(x0), cv(x1), cv(t), cv(z), cv(cond), **lk)
    mean = rows.sum() / (xt.shape[1] * xt.shape[2])
    mean.backward()
    g = {k: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])).detach().numpy().astype(np.float64) for k, _ in spec}
    return rows.detach().numpy().astype(np.float64), float(mean.detach()), g
