#!/usr/bin/env python3
"""Golden vectors for mixed-species batches (tests/test_gpu_species_golden.py): the REFERENCE's own graph construction and drift
networks on one batch whose molecules differ in size, graph and bond types.

Run in the build container only, like make_golden_mask.py (whose shims, radius_graph / coalesce restatements and reference transforms
this imports):
    python tests/golden/make_golden_species.py [--out DIR]

Each molecule goes through the reference's per-sample processing (mdqm9_ambient.py:160-170): COM removal, its own
`AddRadiusGraph(cutoff)`, `AddBondGraph()`, `Coalesce()`, with atom features 0 .. n_b - 1 (the reference's distinguish=True), and the
molecules are collated like a DataLoader batch of PyG: nodes concatenated, edge indices offset by the molecule's first node.
Cases: ambient (F = 32, L = 2, atoms per molecule 5, 9, 7, 9, 5) and latent (F = 32, L = 2, atoms per molecule 4, 7, 6, 6): three
species each, some of them twice.  Bonds are a chain whose types 1-3 start at another type in every species, the last atom has no bond,
and one cutoff for the batch, placed in a gap of the pair distances, keeps about 60 % of the pairs.
Stored, all in the reference's flat node order [N, ..]: the collated graph, the drift of the reference ODEWrapper on the whole mixed
batch at three times, and a hand-rolled fixed-step Euler trajectory over that wrapper on the reference grid.  The reference's
compute_divergence stacks the molecules' coordinates (ode_wrapper.py:75, `torch.stack`) and views the drift as [B, A, 3], so it runs
on equally sized molecules only: it is called once per species, on the collated sub-batch of that species' molecules of the same
mixed batch (molecules do not interact, so this is the mixed batch's divergence), and the values are stored per molecule [B].
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_mask as mm  # noqa: E402  (installs the shims and the two restated torch_geometric functions)

mg, syn, W, OUT = mm.mg, mm.syn, mm.W, mm.OUT


def species_bonds(n):
    """Chain 0 - 1 - .. - (n - 2), both directions, types (i + n) % 3 + 1: another start per species; atom n - 1 has no bond."""
    i = np.arange(n - 2)
    bi = np.stack([np.concatenate([i, i + 1]), np.concatenate([i + 1, i])])
    ty = (i + n) % 3 + 1
    return torch.from_numpy(bi.astype(np.int64)), torch.from_numpy(np.concatenate([ty, ty]).astype(np.int64))


def batch_cutoff(xs, keep):
    """A cutoff in the middle of a gap of all molecules' pair distances near the `keep` quantile."""
    d = np.sort(np.concatenate([np.linalg.norm(x[:, None] - x[None], axis=-1)[~np.eye(len(x), dtype=bool)] for x in xs]))
    k = int(keep * d.size)
    k = max(range(k - 3, k + 4), key=lambda m: d[m + 1] - d[m])
    return float(0.5 * (d[k] + d[k + 1]))


def reference_graph(x, cutoff):
    """The reference's process() transforms on one molecule (already COM-free): (edge_index [2, E] local, edge_type [E])."""
    n = x.shape[0]
    bi, bt = species_bonds(n)
    xb = torch.from_numpy(x)
    one = mg.Batch(x=xb, x0=xb, batch=torch.zeros(n, dtype=torch.long), bond_index=bi, bonds=bt, edge_index=None, edge_type=None)
    one = mm.ref_utils.Coalesce()(mm.ref_utils.AddBondGraph()(mm.ref_utils.AddRadiusGraph(cutoff=cutoff)(one)))
    return one.edge_index, one.edge_type


def collate(variant, mols, which):
    """The PyG collation of the molecules `which` (a list of indices into mols): nodes concatenated, edges offset."""
    xs, ei, et, bidx, ids, cond, first = [], [], [], [], [], [], 0
    for k, b in enumerate(which):
        m = mols[b]
        n = m["x"].shape[0]
        xs.append(torch.from_numpy(m["x"]))
        ei.append(m["edge_index"] + first)
        et.append(m["edge_type"])
        bidx.append(torch.full((n,), k, dtype=torch.long))
        ids.append(torch.arange(n))
        cond.append(torch.from_numpy(m["cond"]))
        first += n
    x, cond = torch.cat(xs), torch.cat(cond)
    kw = dict(x=x.clone(), x0=x.clone(), edge_index=torch.cat(ei, dim=1), edge_type=torch.cat(et), batch=torch.cat(bidx))
    if variant == W.AMBIENT:
        kw.update(atoms=torch.cat(ids), T0=cond[:, 0].clone(), T1=cond[:, 1].clone())
    else:
        kw.update(atom_number=torch.cat(ids), T=cond[:, 0].to(torch.int64))       # reference builds T as int64 (mdqm9_latent.py:184)
    return mg.Batch(**kw)


def species_case(name, variant, F, L, n_atoms, temp_length, *, seed, keep=0.6, traj_steps=4, sigma=0.3):
    B, A = len(n_atoms), max(n_atoms)
    xs = []
    for b, n in enumerate(n_atoms):
        x = syn.molecule_coords(1, n, seed=seed + 10 * b, sigma=sigma)[0]
        xs.append((x - x.mean(axis=0, keepdims=True)).astype(np.float32))
    cutoff = batch_cutoff(xs, keep)
    if variant == W.AMBIENT:
        full = syn.ambient_cond(B, A)
    else:
        full = np.asarray([800.0, 300.0, 1000.0, 500.0], np.float32)[np.arange(B) % 4][:, None, None] * np.ones((B, A, 1), np.float32)
    mols = []
    for b, n in enumerate(n_atoms):
        ei, et = reference_graph(xs[b], cutoff)
        frac = ei.shape[1] / (n * (n - 1))
        assert frac >= 0.3, (b, frac)
        mols.append(dict(x=xs[b], edge_index=ei, edge_type=et, cond=np.ascontiguousarray(full[b, :n])))
    assert len(set(n_atoms)) == 3
    assert sum(m["edge_index"].shape[1] < len(m["x"]) * (len(m["x"]) - 1) for m in mols) >= B - 1      # at most one complete graph
    sd = syn.painn_state_dict(variant, F, L, 25, seed)
    model = mg.build_model(variant, F, L, temp_length, mg.TEMPS, sd)
    Ode = mg.AmbientODE if variant == W.AMBIENT else mg.LatentODE
    batch = collate(variant, mols, list(range(B)))
    ts = np.asarray([0.0, 0.25, 1.0], np.float32)
    out = dict(variant=variant, F=F, L=L, A=A, B=B, seed=seed, temp_length=float(temp_length), temperatures=np.asarray(mg.TEMPS, np.float32),
               n_atoms=np.asarray(n_atoms, np.int32), x=batch.x0.numpy().copy(),
               cond=np.concatenate([m["cond"] for m in mols]), ts=ts, edge_index=batch.edge_index.numpy(), edge_type=batch.edge_type.numpy(),
               batch=batch.batch.numpy(), atom_ids=(batch.atoms if variant == W.AMBIENT else batch.atom_number).numpy())
    ode = Ode(model, return_dlogp=False)
    for i, t in enumerate(ts):
        out[f"drift_{i}"] = mg.drift_via_wrapper(ode, batch, batch.x0.clone(), float(t)).numpy().copy()
    tdiv = float(ts[1])
    out["div_t"] = np.float32(tdiv)
    div = np.zeros(B, np.float32)
    for n in sorted(set(n_atoms)):                            # compute_divergence: one species' molecules at a time (see above)
        which = [b for b in range(B) if n_atoms[b] == n]
        sub = collate(variant, mols, which)
        sub = Ode.reset_batch(sub.clone(), sub.x0.clone(), torch.tensor(tdiv))
        div[which] = Ode.compute_divergence(model, sub).detach().numpy()           # ambient: * 1e-2 like the reference
    out["div"] = div
    grid, path = mg.rollout_reference(ode, batch, traj_steps, "euler")
    out["traj_grid"], out["traj_euler"] = grid, path
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    counts = [int(m["edge_index"].shape[1]) for m in mols]
    print(f"{name}: cutoff {cutoff:.4f}, atoms {list(n_atoms)}, edges per molecule {counts}, div {div}, "
          f"size={os.path.getsize(os.path.join(OUT, name + '.npz')) / 1024:.0f} KiB")


if __name__ == "__main__":
    torch.set_num_threads(8)
    species_case("species_ambient", W.AMBIENT, 32, 2, (5, 9, 7, 9, 5), 100, seed=60)
    species_case("species_latent", W.LATENT_MULTI, 32, 2, (4, 7, 6, 6), 75, seed=61)
