#!/usr/bin/env python3
"""Generate tests/golden/painn_train_{ambient,latent}.npz: the REFERENCE's gradients of the velocity loss with respect to every
parameter of cPaiNN (mdqm9/thermo/{ambient,latent}: models/cpainn.py under losses.py's make_batch_loss), by its own autograd, at the
recorded (t, z) of the vloss fixtures and at their shapes (F 32, L 2, A 6, B 5 and B 4).  Ambient: the three gamma kinds of the
standard loss; latent: the one-sided loss at both t_distr draws.  Per case: the loss rows and their mean from the float32 model and from
the same model in .double() on the same float32 states, the gradient of the mean per state_dict key from the double model (g64::), and
beside it the float32 model's own rel-L2 distance from it per tensor (d32::).  A file stays below 1 MiB, so the ambient cases sin2 and
sig_sum and the gradients of the second and third optimiser step lie in files of their own (painn_train_ambient_{sin2,sig_sum,steps}.npz).  The states
are the fp64 interpolation of tests/vloss_numpy.py rounded to float32 once -- what the device evaluates; the vloss fixtures pin that
restatement against the reference's interpolants.  For the ambient brownian case also three optimiser steps of the .double() model
(clip_grad_norm_ 1, torch.optim.Adam lr 1e-4) on that batch: the gradient of every step and the weights after the third, with the
clip active (asserted here).  The inputs of the ambient cases are the vloss fixture's coordinates scaled by X_SCALE, the scale at which
the untrained model's gradient norm exceeds 1.  Imports the reference modules, stores none of their text.  Run in the build container
only:
    python tests/golden/make_golden_painn_train.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import vloss_numpy as vn  # noqa: E402
import make_golden as mg  # noqa: E402
from thermo.ambient import interpolants as amb_i, losses as amb_l  # noqa: E402
from thermo.latent import interpolants as lat_i, losses as lat_l  # noqa: E402

W, syn = mg.W, mg.syn
X_SCALE = 4.0


def load(name):
    with np.load(os.path.join(HERE, name)) as z:
        return {k: z[k] for k in z.files}


def run(model, loss_fn, variant, g, x0n, x1n, t, z, kind, gamma, a, dtype):
    """One forward and backward pass of the reference at given states -> (rows [B], {key: grad})"""
    B, A = x0n.shape[:2]
    src, dst, etype, ids, cond = g["edge_src"], g["edge_dst"], g["edge_type"], g["atom_ids"], g["cond"]
    xt, _ = vn.interpolate(x0n, x1n, t, z, kind=kind, gamma_kind=gamma, a=a, center="batch")
    xt = xt.astype(np.float32)
    cast = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
    torch.set_default_dtype(dtype)              # the model's own zeros and aranges follow the default type
    zeros = torch.zeros                         # the latent model's equivariant features are zeros of an explicit float32
    torch.zeros = lambda *ar, **kw: zeros(*ar, **{**kw, "dtype": dtype if kw.get("dtype") == torch.float32 else kw.get("dtype")})
    for mod in model.modules():                 # ... and its temperature ladder is a float32 tensor outside the state_dict
        if isinstance(getattr(mod, "temperatures", None), torch.Tensor):
            mod.temperatures = mod.temperatures.to(dtype)
    model.zero_grad()
    outs = []
    for half in range(xt.shape[0]):
        b = mg.make_batch(variant, xt[half], cond, src, dst, etype, ids)
        b.x, b.x0 = cast(xt[half].reshape(B * A, 3)), cast(x0n.reshape(B * A, 3))
        b.t = cast(np.repeat(t, A))
        if variant == W.AMBIENT:
            b.T0, b.T1 = b.T0.to(dtype), b.T1.to(dtype)
        outs.append(model(b).output)
    f = lambda v: cast(np.asarray(v).reshape(B * A, -1))
    zz = f(z) if z is not None else torch.zeros(B * A, 3, dtype=dtype)
    rows = loss_fn.make_batch_loss()(f(np.repeat(t, A)), zz, f(x0n), f(x1n), outs[0], outs[-1])
    rows.mean().backward()
    torch.set_default_dtype(torch.float32)
    torch.zeros = zeros
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().numpy().copy() for k, p in model.named_parameters()
             if not k.endswith("device_tracker")}
    return rows.detach().double().numpy().reshape(B, A).sum(axis=1), grads


def store(out, case, tag, rows, grads, n_rows, keep):
    """rows and mean of either model; the float64 gradients in full, and beside them the float32 model's rel-L2 distance per tensor
    (d32::, -1 where the float64 gradient is all zero and the float32 one is not)"""
    out.update({f"{case}::rows{tag}": rows, f"{case}::mean{tag}": float(rows.sum() / n_rows)})
    if tag == "32":
        keep.update(grads)
        return
    for k, v in grads.items():
        out[f"{case}::g64::{k}"] = v
        nr = np.linalg.norm(v)
        out[f"{case}::d32::{k}"] = float(np.linalg.norm(keep[k] - v) / nr) if nr > 0 else (-1.0 if np.any(keep[k]) else 0.0)


def main():
    F, L = 32, 2
    # ---- ambient
    g = load("vloss_ambient.npz")
    A, B, seed = int(g["A"]), int(g["B"]), int(g["seed"])
    x0n, x1n = (X_SCALE * g["x0"]).astype(np.float32), (X_SCALE * g["x1"]).astype(np.float32)
    sd = syn.painn_state_dict(W.AMBIENT, F, L, 25, seed)
    out = {k: g[k] for k in ("variant", "F", "L", "A", "B", "seed", "temp_length", "temperatures", "edge_src", "edge_dst", "edge_type", "atom_ids",
                             "cond", "cases", "a")}
    out.update(x0=x0n, x1=x1n, x_scale=X_SCALE)
    for case, a in zip(g["cases"], g["a"]):
        case, a = str(case), float(a)
        t, z = g[f"{case}::t"], g[f"{case}::z"]
        out.update({f"{case}::t": t, f"{case}::z": z})
        side, keep = {}, {}
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            model = mg.build_model(W.AMBIENT, F, L, 100, mg.TEMPS, sd).to(dtype)
            loss_fn = amb_l.StandardVelocityLoss(amb_i.LinearInterpolant(a=a, gamma=case), t_distr="uniform")
            rows, grads = run(model, loss_fn, W.AMBIENT, g, x0n, x1n, t, z, "standard", case, a, dtype)
            store(side if case != "brownian" else out, case, tag, rows, grads, B * A, keep)
            print(f"ambient {case} float{tag}: mean {rows.sum() / (B * A):.7f}  |g| {np.sqrt(sum((v * v).sum() for v in grads.values())):.4f}")
        if side:
            np.savez_compressed(os.path.join(HERE, f"painn_train_ambient_{case}.npz"), **side)
    # three optimiser steps of the double model on the brownian case
    case, a = "brownian", float(g["a"][0])
    t, z = g[f"{case}::t"], g[f"{case}::z"]
    model = mg.build_model(W.AMBIENT, F, L, 100, mg.TEMPS, sd).double()
    params = [p for k, p in model.named_parameters() if not k.endswith("device_tracker")]
    opt = torch.optim.Adam(params, lr=1e-4)
    loss_fn = amb_l.StandardVelocityLoss(amb_i.LinearInterpolant(a=a, gamma=case), t_distr="uniform")
    clipped, steps = [], {}
    for k in range(3):
        opt.zero_grad()
        rows, grads = run(model, loss_fn, W.AMBIENT, g, x0n, x1n, t, z, "standard", case, a, torch.float64)
        norm = float(torch.nn.utils.clip_grad_norm_(params, 1.0))
        clipped.append(norm > 1.0)
        if k == 0:                                   # the first step's gradient is the brownian case's g64, bit for bit
            assert all(np.array_equal(v, out[f"brownian::g64::{key}"]) for key, v in grads.items())
        else:
            steps.update({f"steps::{k}::g::{key}": v for key, v in grads.items()})
        out[f"steps::{k}::gnorm"] = norm
        opt.step()
        print(f"step {k}: mean {rows.sum() / (B * A):.7f}  |g| {norm:.4f}")
    assert any(clipped), "the clip is never active: raise X_SCALE"
    out.update({f"steps::w::{k}": p.detach().numpy().copy() for k, p in model.named_parameters() if not k.endswith("device_tracker")})
    out["steps::lr"] = 1e-4
    np.savez_compressed(os.path.join(HERE, "painn_train_ambient.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "painn_train_ambient_steps.npz"), **steps)

    # ---- latent, several temperatures: the one-sided loss
    g = load("vloss_latent_multi.npz")
    A, B, seed = int(g["A"]), int(g["B"]), int(g["seed"])
    sd = syn.painn_state_dict(W.LATENT_MULTI, F, L, 25, seed)
    out = {k: g[k] for k in ("variant", "F", "L", "A", "B", "seed", "temp_length", "temperatures", "edge_src", "edge_dst", "edge_type", "atom_ids",
                             "cond", "cases", "x0", "x1")}
    for case in g["cases"]:
        case = str(case)
        t = g[f"{case}::t"]
        out[f"{case}::t"] = t
        keep = {}
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            model = mg.build_model(W.LATENT_MULTI, F, L, 75, mg.TEMPS, sd).to(dtype)
            loss_fn = lat_l.OneSidedVelocityLoss(lat_i.OneSidedLinearInterpolant(), t_distr=case)
            rows, grads = run(model, loss_fn, W.LATENT_MULTI, g, g["x0"], g["x1"], t, None, "one_sided", "brownian", 1.0, dtype)
            store(out, case, tag, rows, grads, B * A, keep)
            print(f"latent {case} float{tag}: mean {rows.sum() / (B * A):.7f}  |g| {np.sqrt(sum((v * v).sum() for v in grads.values())):.4f}")
    np.savez_compressed(os.path.join(HERE, "painn_train_latent.npz"), **out)


if __name__ == "__main__":
    main()
