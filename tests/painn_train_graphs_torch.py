"""The torch restatement of the molecule trainer on per-molecule graphs (ti_painn_train_set_graphs): every molecule of a padded batch
goes through painn_train_torch.forward on its OWN sub-template -- its n_b atoms, its live edges in template order, its types -- so
molecules do not interact and nothing of a pad or a dead edge exists; the loss is summed over the real entries and divided by
N = sum_b n_b.  tests/test_painn_train_graphs_host.py pins it against the reference's own gradients on mixed batches,
tests/test_gpu_painn_train_graphs.py compares the device gradients with it."""
import numpy as np
import torch

import painn_train_torch as ptt
import vloss_numpy as vn


def live_edges(model, n, mask_row, ptype_b):
    """(src, dst, etype) of one molecule: the template's edges, in template order, that lie between its n real atoms and whose bit is
    set (mask_row [A] uint32 | None: all), with its own types (ptype_b [A, A] | None: the template's)"""
    src, dst, et = (np.asarray(model[k], np.int64) for k in ("src", "dst", "etype"))
    keep = (src < n) & (dst < n)
    if mask_row is not None:
        keep &= ((np.asarray(mask_row, np.uint32)[dst] >> src.astype(np.uint32)) & np.uint32(1)).astype(bool)
    if ptype_b is not None:
        et = np.asarray(ptype_b, np.int64)[src, dst]
    return src[keep], dst[keep], et[keep]


def states(x0, x1, t, z, n_atoms, kind="standard", gamma="brownian", a=1.0, center="batch"):
    """xt [halves, B, A, 3] float32 on the real entries (pads 0): the fp64 interpolation, centred over the N real node rows (batch),
    over a molecule's n_b atoms (molecule) or not at all, rounded to float32 once"""
    B, A = x0.shape[:2]
    real = np.arange(A)[None, :] < np.asarray(n_atoms)[:, None]               # [B, A]
    x0, x1 = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    tt = np.asarray(t, np.float64)[:, None, None]
    if kind == "one_sided":
        xs = [tt * x1 + (1.0 - tt) * x0]
    else:
        it, gz = (1.0 - tt) * x0 + tt * x1, vn.gamma(gamma, a, tt) * np.asarray(z, np.float64)
        xs = [it + gz, it - gz]
    out = []
    for x in xs:
        x = np.where(real[..., None], x, 0.0)
        if center == "batch":
            x = x - x.sum(axis=(0, 1)) / real.sum()
        elif center == "molecule":
            x = x - x.sum(axis=1, keepdims=True) / np.asarray(n_atoms, np.float64)[:, None, None]
        out.append(np.where(real[..., None], x, 0.0))
    return np.stack(out).astype(np.float32)


def grads(flat, spec, model, n_atoms, mask, pair_type, xt, x0, x1, t, z, cond, dtype=torch.float64, kind="standard", gamma="brownian", a=1.0):
    """-> (loss rows [B], mean, {key: gradient of the mean}, drift [halves, B, A, 3] with 0 on pads) with every input cast to `dtype`.
    The arrays are padded [B, A, ..]; pad entries are never read."""
    P, o = {}, 0
    for k, shape in spec:
        n = int(np.prod(shape))
        P[k] = torch.tensor(np.asarray(flat[o:o + n], np.float64).reshape(shape), dtype=dtype, requires_grad=True)
        o += n
    cv = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=dtype)
    halves, B, A = xt.shape[:3]
    base = {k: v for k, v in model.items() if k not in ("src", "dst", "etype", "atom_ids")}
    rows, drift = [], torch.zeros(halves, B, A, 3, dtype=dtype)
    for b in range(B):
        n = int(n_atoms[b])
        s, d, e = live_edges(model, n, None if mask is None else mask[b], None if pair_type is None else pair_type[b])
        cb = None if cond is None else cv(cond[b, :n])[None].repeat(halves, 1, 1)
        out = ptt.forward(P, src=s, dst=d, etype=e, atom_ids=np.asarray(model["atom_ids"])[:n], x=cv(xt[:, b, :n]), t=cv(t[b:b + 1]).repeat(halves),
                          cond=cb, **base)                               # [halves, n, 3]
        dlt = cv(x1[b, :n]) - cv(x0[b, :n])
        if kind == "one_sided":
            rows.append((0.5 * out[0] * out[0] - dlt * out[0]).sum())
        else:
            gz = ptt.gamma_dot(gamma, a, cv(t[b:b + 1])) * cv(z[b, :n])
            rows.append((0.5 * out[0] * out[0] - (dlt + gz) * out[0] + 0.5 * out[1] * out[1] - (dlt - gz) * out[1]).sum())
        drift[:, b, :n] = out.detach()
    rows = torch.stack(rows)
    mean = rows.sum() / int(np.sum(n_atoms))
    mean.backward()
    g = {k: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])).detach().numpy().astype(np.float64) for k, _ in spec}
    return rows.detach().numpy().astype(np.float64), float(mean.detach()), g, drift.numpy().astype(np.float64)
