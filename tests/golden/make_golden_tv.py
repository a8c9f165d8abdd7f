#!/usr/bin/env python3
"""Generate tests/golden/tv_*.npz: the REFERENCE drift networks evaluated at one time per molecule (cPaiNN, batch.t per node,
constant within a molecule) and one time per row (FCNetMultiBeta, ts [B, 1]) -- the inputs the reference's training losses feed
(mdqm9/thermo/ambient/losses.py:45-70).  Reuses make_golden.py's shims and helpers; run in the build container only:
    python tests/golden/make_golden_tv.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shims and imports the reference modules)

W, syn = mg.W, mg.syn


def painn_tv_case(name, variant, F, L, A, B, temp_length, temperatures, *, seed, sigma=0.3, with_div=False):
    src, dst, etype = syn.fully_connected_template(A)
    atom_ids = np.arange(A, dtype=np.int32)
    x = syn.molecule_coords(B, A, seed=seed, sigma=sigma)
    if variant == W.AMBIENT:
        cond = syn.ambient_cond(B, A)
    else:
        cond = np.asarray([800.0, 300.0, 1000.0, 500.0], np.float32)[np.arange(B) % 4][:, None, None] * np.ones((B, A, 1), np.float32)
    tv = np.linspace(0.05, 0.95, B).astype(np.float32)[np.random.RandomState(seed).permutation(B)]
    sd = syn.painn_state_dict(variant, F, L, 25, seed)
    model = mg.build_model(variant, F, L, temp_length, temperatures, sd)
    batch = mg.make_batch(variant, x, cond, src, dst, etype, atom_ids)
    b = batch.clone()
    b.t = torch.from_numpy(np.repeat(tv, A))                    # batch.t per node, one value per molecule
    with torch.no_grad():
        drift = model(b).output.numpy().reshape(B, A, 3).copy()
    out = dict(variant=variant, F=F, L=L, A=A, B=B, seed=seed, temp_length=float(temp_length),
               temperatures=np.asarray(temperatures, np.float32), edge_src=src, edge_dst=dst, edge_type=etype, atom_ids=atom_ids,
               x=x, cond=cond, tv=tv, drift_tv=drift)
    if with_div:                                                 # ODEWrapper.compute_divergence at the per-molecule batch.t
        ode_cls = mg.AmbientODE if variant == W.AMBIENT else mg.LatentODE
        d = batch.clone()
        d.t = torch.from_numpy(np.repeat(tv, A))
        out["div_tv"] = ode_cls.compute_divergence(model, d).detach().numpy().reshape(B).copy()
    np.savez_compressed(os.path.join(mg.HERE, name + ".npz"), **out)
    print(f"{name}: |b|={np.linalg.norm(drift):.5f}")


def adw_tv_case(name, hidden, layers, B, *, seed):
    x = syn.adw_x0(B, seed)
    rs = np.random.RandomState(seed + 100)
    beta0 = rs.choice([0.25, 0.5, 0.75, 1.0], B)
    beta1 = rs.choice([0.5, 1.0, 1.25, 1.5], B)
    tv = rs.uniform(0.0, 1.0, B).astype(np.float32)
    model = mg.adw_simple.FCNetMultiBeta(1, 1, hidden, layers).double()
    model.load_state_dict(mg.to_torch_sd(syn.adw_state_dict(hidden, layers, seed)))
    model.eval()
    col = lambda a: torch.from_numpy(np.asarray(a, np.float64))[:, None]
    with torch.no_grad():
        drift = model(None, col(x), col(tv), col(beta0), col(beta1)).numpy()[:, 0].copy()
    np.savez_compressed(os.path.join(mg.HERE, name + ".npz"), hidden=hidden, num_layers=layers, B=B, seed=seed, x=x, beta0=beta0,
                        beta1=beta1, tv=tv, drift_tv=drift)
    print(f"{name}: |b|={np.linalg.norm(drift):.5f}")


if __name__ == "__main__":
    TEMPS = mg.TEMPS
    painn_tv_case("tv_ambient", W.AMBIENT, 32, 2, 6, 5, 100, TEMPS, seed=11, with_div=True)
    painn_tv_case("tv_latent_multi", W.LATENT_MULTI, 32, 2, 6, 4, 75, TEMPS, seed=12, sigma=1.0)
    adw_tv_case("tv_adw_h64", 64, 3, 32, seed=13)
