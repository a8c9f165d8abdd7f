#!/usr/bin/env python3
"""Generate tests/golden/painn_train_graphs_{ambient,latent}.npz: the REFERENCE's gradients of the velocity loss on ONE MIXED batch per
variant family -- molecules of different size, each with its own radius graph and bond types -- by its own autograd on its .double()
model, with the float32 model's per-tensor distance beside them (d32::), as make_golden_painn_train.py stores them for uniform batches.

Run in the build container only, like make_golden_species.py (whose collate, chain bonds and batch cutoff this imports, with the shims
of make_golden_mask.py behind them):
    python tests/golden/make_golden_painn_train_graphs.py

Ambient: the standard loss (brownian, a = 0.9), atoms per molecule (5, 3, 4, 5).  Latent, several temperatures: the one-sided loss,
atoms (4, 2, 3).  Both F 32, L 2, recorded (t, z).  Every molecule goes through the reference's per-sample transforms on its set-0
sample (AddRadiusGraph at one batch cutoff that keeps about 60 % of the pairs, AddBondGraph with chain bonds whose types start
differently per species, Coalesce) and the molecules are collated like a PyG batch; both states xt+ and xt- are evaluated on that graph,
as the reference's loss does (losses.py:58-59).  The states are interpolated and batch-centred in fp64 over the real rows -- the mean
over the flat [N, 3] -- and rounded to float32 once: what the device evaluates.  Stored in the reference's flat node order: the collated
graph, x0, x1, cond [N, ..], t [B], z [N, 3]; rows and mean of either model (rows summed per molecule, mean = sum / N); g64:: and d32::
per state_dict key.  Imports the reference modules, stores none of their text."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_species as ms  # noqa: E402  (make_golden_mask's shims, collate, species_bonds, batch_cutoff)
import painn_train_graphs_torch as pgt  # noqa: E402
from thermo.ambient import interpolants as amb_i, losses as amb_l  # noqa: E402
from thermo.latent import interpolants as lat_i, losses as lat_l  # noqa: E402

mg, syn, W = ms.mg, ms.syn, ms.W


def states(x0, x1, t, z, n_atoms, kind, gamma, a):
    """xt [halves, N, 3] float32: the fp64 interpolation over the flat real rows, centred on their mean, rounded once -- by the
    restatement's own function on the padded layout, so that the test evaluates the very states the reference was given"""
    B, A = len(n_atoms), max(n_atoms)
    real = np.arange(A)[None, :] < np.asarray(n_atoms)[:, None]

    def pad(v):
        out = np.zeros((B, A, 3), np.float32)
        out[real] = v
        return out

    xt = pgt.states(pad(x0), pad(x1), t, None if z is None else pad(z), n_atoms, kind=kind, gamma=gamma, a=a, center="batch")
    return np.ascontiguousarray(xt[:, real])


def run(model, loss_fn, variant, mols, xt, x0, x1, t_node, z, dtype):
    """One forward and backward pass of the reference on the collated batch at given states -> (rows per node [N], {key: grad})"""
    cast = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
    torch.set_default_dtype(dtype)
    zeros = torch.zeros
    torch.zeros = lambda *ar, **kw: zeros(*ar, **{**kw, "dtype": dtype if kw.get("dtype") == torch.float32 else kw.get("dtype")})
    for mod in model.modules():
        if isinstance(getattr(mod, "temperatures", None), torch.Tensor):
            mod.temperatures = mod.temperatures.to(dtype)
    model.zero_grad()
    outs = []
    for half in range(xt.shape[0]):
        b = ms.collate(variant, mols, list(range(len(mols))))
        b.x, b.x0 = cast(xt[half]), cast(x0)
        b.t = cast(t_node)
        if variant == W.AMBIENT:
            b.T0, b.T1 = b.T0.to(dtype), b.T1.to(dtype)
        outs.append(model(b).output)
    zz = cast(z) if z is not None else torch.zeros(x0.shape[0], 3, dtype=dtype)
    rows = loss_fn.make_batch_loss()(cast(t_node[:, None]), zz, cast(x0), cast(x1), outs[0], outs[-1])
    rows.mean().backward()
    torch.set_default_dtype(torch.float32)
    torch.zeros = zeros
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().numpy().copy() for k, p in model.named_parameters()
             if not k.endswith("device_tracker")}
    return rows.detach().double().numpy().reshape(-1), grads


def case(name, variant, n_atoms, temp_length, kind, gamma, a, seed, keep=0.6):
    F, L, B, A = 32, 2, len(n_atoms), max(n_atoms)
    rs = np.random.RandomState(seed)
    x0s, x1s = [], []
    for b, n in enumerate(n_atoms):
        shape = syn.molecule_coords(1, n, seed=seed + 10 * b, sigma=0.3)[0]
        for xs, shift in ((x0s, 0.0), (x1s, 0.4)):
            x = shape * (1.0 + shift) + 0.1 * rs.standard_normal((n, 3))
            xs.append((x - x.mean(axis=0, keepdims=True)).astype(np.float32))
    cutoff = ms.batch_cutoff(x0s, keep)
    if variant == W.AMBIENT:
        full = syn.ambient_cond(B, A)
    else:
        full = np.asarray([800.0, 300.0, 1000.0], np.float32)[np.arange(B) % 3][:, None, None] * np.ones((B, A, 1), np.float32)
    mols = []
    for b, n in enumerate(n_atoms):
        ei, et = ms.reference_graph(x0s[b], cutoff)            # batch0's graph
        mols.append(dict(x=x0s[b], edge_index=ei, edge_type=et, cond=np.ascontiguousarray(full[b, :n])))
    x0, x1 = np.concatenate(x0s), np.concatenate(x1s)
    N = x0.shape[0]
    t = (0.15 + 0.7 * rs.random_sample(B)).astype(np.float32)
    t_node = np.repeat(t, n_atoms)
    z = rs.standard_normal((N, 3)).astype(np.float32) if kind == "standard" else None
    xt = states(x0, x1, t, z, n_atoms, kind, gamma, a)
    sd = syn.painn_state_dict(variant, F, L, 25, seed)
    batch = ms.collate(variant, mols, list(range(B)))
    out = dict(variant=variant, F=F, L=L, A=A, B=B, seed=seed, temp_length=float(temp_length), temperatures=np.asarray(mg.TEMPS, np.float32),
               n_atoms=np.asarray(n_atoms, np.int32), x0=x0, x1=x1, cond=np.concatenate([m["cond"] for m in mols]), t=t, cutoff=cutoff,
               edge_index=batch.edge_index.numpy(), edge_type=batch.edge_type.numpy(), batch=batch.batch.numpy(), kind=kind, gamma=gamma, a=a)
    if z is not None:
        out["z"] = z
    first = np.concatenate([[0], np.cumsum(n_atoms)[:-1]])
    keep32 = {}
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        model = mg.build_model(variant, F, L, temp_length, mg.TEMPS, sd).to(dtype)
        if variant == W.AMBIENT:
            loss_fn = amb_l.StandardVelocityLoss(amb_i.LinearInterpolant(a=a, gamma=gamma), t_distr="uniform")
        else:
            loss_fn = lat_l.OneSidedVelocityLoss(lat_i.OneSidedLinearInterpolant(), t_distr="uniform")
        rows, grads = run(model, loss_fn, variant, mols, xt, x0, x1, t_node, z, dtype)
        out[f"rows{tag}"], out[f"mean{tag}"] = np.add.reduceat(rows, first), float(rows.sum() / N)
        if tag == "32":
            keep32 = grads
            continue
        for k, v in grads.items():
            out[f"g64::{k}"] = v
            nr = np.linalg.norm(v)
            out[f"d32::{k}"] = float(np.linalg.norm(keep32[k] - v) / nr) if nr > 0 else (-1.0 if np.any(keep32[k]) else 0.0)
        print(f"{name} float{tag}: mean {rows.sum() / N:.7f}  |g| {np.sqrt(sum((v * v).sum() for v in grads.values())):.4f}")
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    counts = [int(m["edge_index"].shape[1]) for m in mols]
    print(f"{name}: cutoff {cutoff:.4f}, atoms {list(n_atoms)}, edges per molecule {counts}, size {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    torch.set_num_threads(8)
    # a as the reference holds it: float32
    case("painn_train_graphs_ambient", W.AMBIENT, (5, 3, 4, 5), 100, "standard", "brownian", float(np.float32(0.9)), seed=70)
    case("painn_train_graphs_latent", W.LATENT_MULTI, (4, 2, 3), 75, "one_sided", "brownian", 1.0, seed=71)
