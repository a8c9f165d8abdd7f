#!/usr/bin/env python3
"""Golden vectors for per-molecule edge sets (tests/test_gpu_edge_mask.py): the REFERENCE's own graph construction and drift networks
on a batch whose molecules have different radius graphs (a finite `cutoff`).

Run in the build container only, like make_golden.py (whose shims and helpers this imports):
    python tests/golden/make_golden_mask.py [--out DIR] [--f256-only]

--out DIR writes the fixtures into DIR instead of tests/golden (make_golden.py reads the flag); --f256-only writes only the two
fixtures at the mdqm9 configs' width.

Each molecule goes through the reference's per-sample processing (mdqm9_ambient.py:160-170): COM removal, then its own
`AddRadiusGraph(cutoff)`, `AddBondGraph()`, `Coalesce()` (mdqm9/thermo/utils.py), and the molecules are collated like a DataLoader
batch (edge indices offset by the molecule's first node).  torch_geometric is absent here: besides make_golden.py's two shims, the two
functions those transforms call are restated from their documented semantics -- `radius_graph(x, r, batch)` (ordered pairs j -> i,
i != j, same molecule, |x_i - x_j| <= r; the cutoff is placed in a gap of the distances, so < and <= agree) and
`utils.coalesce(edge_index, edge_attr, reduce="max")` (sort by (row, col), merge duplicates with max).
Cases: ambient (F = 32, L = 2, A = 9, B = 4) and latent (F = 32, L = 2, A = 7, B = 3); with --f256-only, ambient (F = 256, L = 5, A = 25,
B = 3) and latent (F = 256, L = 5, A = 18, B = 3, coordinates with sigma 0.5 as in make_golden.py's latent_f256: at unit variance the
reference's own fp32 drift misses the 1e-5 bar).  The F = 256 divergence is taken on one thread: on several, the reference's autograd
divergence changes in its last bits from run to run (make_golden.py --f256-only does the same).  The cutoff keeps 40-80 % of the pairs, bonds are
a chain with types 1-3 and the last atom has no bond; in molecule 0 that atom sits far from the others and has no incoming edge.
Stored: the collated graph, the drift of the reference ODEWrapper at three times, the reference compute_divergence (autograd), and a
hand-rolled fixed-step Euler trajectory over the wrapper on the reference grid.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the shims, imports the reference modules)

OUT = mg.OUT
syn, W = mg.syn, mg.W


def radius_graph(x, r, batch=None, max_num_neighbors=32, loop=False, flow="source_to_target"):
    assert not loop and flow == "source_to_target"
    batch = torch.zeros(x.shape[0], dtype=torch.long) if batch is None else batch
    d = torch.cdist(x.double(), x.double())
    ok = (d <= r) & (batch[:, None] == batch[None, :]) & ~torch.eye(x.shape[0], dtype=torch.bool)
    i, j = torch.nonzero(ok, as_tuple=True)                 # i: target (centre), j: source (neighbour)
    return torch.stack([j, i])


def coalesce(edge_index, edge_attr, reduce="max"):
    assert reduce == "max"
    n = int(edge_index.max()) + 1
    key = edge_index[0] * n + edge_index[1]
    uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
    out = torch.full((uniq.numel(),), torch.iinfo(torch.long).min, dtype=torch.long).scatter_reduce(0, inv, edge_attr, reduce="amax")
    return torch.stack([uniq // n, uniq % n]), out


tg = sys.modules["torch_geometric"]
tg.nn = type(sys)("torch_geometric.nn")
tg.nn.radius_graph = radius_graph
tg.utils = type(sys)("torch_geometric.utils")
tg.utils.coalesce = coalesce
sys.modules["torch_geometric.nn"], sys.modules["torch_geometric.utils"] = tg.nn, tg.utils
from thermo import utils as ref_utils  # noqa: E402  (mdqm9/thermo/utils.py)


def chain_bonds(A):
    i = np.arange(A - 2)
    bi = np.stack([np.concatenate([i, i + 1]), np.concatenate([i + 1, i])])
    return torch.from_numpy(bi.astype(np.int64)), torch.from_numpy(np.concatenate([i % 3 + 1, i % 3 + 1]).astype(np.int64))


def gap_cutoff(x, keep):
    """A cutoff in the middle of a gap of the pair distances of molecules 1.. near the `keep` quantile."""
    A = x.shape[1]
    d = np.sort(np.linalg.norm(x[:, :, None] - x[:, None, :], axis=-1)[1:][:, ~np.eye(A, dtype=bool)].ravel())
    k = int(keep * d.size)
    k = max(range(k - 3, k + 4), key=lambda m: d[m + 1] - d[m])
    return float(0.5 * (d[k] + d[k + 1]))


def reference_graphs(x, cutoff, bond_index, bonds):
    """Per molecule: the reference's process() transforms on a one-molecule batch; collated with node offsets."""
    B, A, _ = x.shape
    ei, et = [], []
    for b in range(B):
        xb = torch.from_numpy(x[b])
        xb = xb - torch.mean(xb, dim=0)
        one = mg.Batch(x=xb, x0=xb, batch=torch.zeros(A, dtype=torch.long), bond_index=bond_index, bonds=bonds, edge_index=None, edge_type=None)
        one = ref_utils.AddRadiusGraph(cutoff=cutoff)(one)
        one = ref_utils.AddBondGraph()(one)
        one = ref_utils.Coalesce()(one)
        ei.append(one.edge_index + b * A)
        et.append(one.edge_type)
    return torch.cat(ei, dim=1), torch.cat(et)


def mask_case(name, variant, F, L, A, B, temp_length, *, seed, keep=0.45, traj_steps=4, sigma=0.3, div_threads=None):
    x = syn.molecule_coords(B, A, seed=seed, sigma=sigma)
    x[0, A - 1] += 25.0                                      # molecule 0: the bond-free last atom far away -> no incoming edge
    x = (x - x.mean(axis=1, keepdims=True)).astype(np.float32)
    cutoff = gap_cutoff(x, keep)
    bi, bt = chain_bonds(A)
    edge_index, edge_type = reference_graphs(x, cutoff, bi, bt)
    mol = edge_index[0] // A
    counts = np.bincount(mol.numpy(), minlength=B)
    assert len(set(counts.tolist())) > 1, counts                  # the molecules really have different graphs
    assert not ((edge_index[1] == A - 1) & (mol == 0)).any(), "molecule 0's last atom must have no incoming edge"
    frac = counts[1:] / (A * (A - 1))
    assert (frac >= 0.4).all() and (frac <= 0.8).all(), frac
    if variant == W.AMBIENT:
        cond = syn.ambient_cond(B, A)
    else:
        cond = np.asarray([800.0, 300.0, 1000.0, 500.0], np.float32)[np.arange(B) % 4][:, None, None] * np.ones((B, A, 1), np.float32)
    sd = syn.painn_state_dict(variant, F, L, 25, seed)
    model = mg.build_model(variant, F, L, temp_length, mg.TEMPS, sd)
    N = B * A
    kw = dict(x=torch.from_numpy(x.reshape(N, 3).copy()), x0=torch.from_numpy(x.reshape(N, 3).copy()), edge_index=edge_index,
              edge_type=edge_type, batch=torch.arange(B).repeat_interleave(A))
    ids = torch.arange(A).repeat(B)
    if variant == W.AMBIENT:
        kw.update(atoms=ids, T0=torch.from_numpy(cond[..., 0].reshape(N).copy()), T1=torch.from_numpy(cond[..., 1].reshape(N).copy()))
        Ode = mg.AmbientODE
    else:
        kw.update(atom_number=ids, T=torch.from_numpy(cond[..., 0].reshape(N).astype(np.int64)))
        Ode = mg.LatentODE
    batch = mg.Batch(**kw)
    ts = np.asarray([0.0, 0.25, 1.0], np.float32)
    out = dict(variant=variant, F=F, L=L, A=A, B=B, seed=seed, temp_length=float(temp_length), temperatures=np.asarray(mg.TEMPS, np.float32),
               cutoff=np.float32(cutoff), x=x, cond=cond, ts=ts, edge_index=edge_index.numpy(), edge_type=edge_type.numpy(),
               batch=kw["batch"].numpy(), atom_ids=ids.numpy(), bond_index=bi.numpy(), bonds=bt.numpy())
    ode = Ode(model, return_dlogp=False)
    for i, t in enumerate(ts):
        out[f"drift_{i}"] = mg.drift_via_wrapper(ode, batch, batch.x0.clone(), float(t)).numpy().reshape(B, A, 3).copy()
    tdiv = float(ts[1])
    b2 = Ode.reset_batch(batch.clone(), batch.x0.clone(), torch.tensor(tdiv))
    out["div_t"] = np.float32(tdiv)
    nt = torch.get_num_threads()
    torch.set_num_threads(div_threads or nt)
    out["div"] = Ode.compute_divergence(model, b2).detach().numpy().copy()          # ambient: * 1e-2 like the reference
    torch.set_num_threads(nt)
    grid, path = mg.rollout_reference(ode, batch, traj_steps, "euler")
    out["traj_grid"], out["traj_euler"] = grid, path.reshape(traj_steps, B, A, 3)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: cutoff {cutoff:.4f}, edges per molecule {counts.tolist()}, div {out['div']}, "
          f"size={os.path.getsize(os.path.join(OUT, name + '.npz')) / 1024:.0f} KiB")


if __name__ == "__main__":
    torch.set_num_threads(8)
    if "--f256-only" in sys.argv:       # the mdqm9 configs' width: n_features 256, score_layers 5
        mask_case("mask_ambient_f256", W.AMBIENT, 256, 5, 25, 3, 100, seed=52, div_threads=1)
        mask_case("mask_latent_f256", W.LATENT_MULTI, 256, 5, 18, 3, 75, seed=53, sigma=0.5, div_threads=1)
        sys.exit(0)
    mask_case("mask_ambient", W.AMBIENT, 32, 2, 9, 4, 100, seed=50)
    mask_case("mask_latent", W.LATENT_MULTI, 32, 2, 7, 3, 75, seed=51)
