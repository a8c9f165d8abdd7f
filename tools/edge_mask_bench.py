#!/usr/bin/env python3
"""Cost of per-molecule edge sets (ti_painn_set_edge_mask) at the headline shape: 65 536 x 18 atoms, F = 128, L = 5, f16x2, EM steps
on device-resident buffers, in three cases -- no mask, an all-ones mask, a radius mask keeping about half the pairs -- and the exact
divergence (54 tangent directions per molecule) with and without a radius mask.  Prints one JSON line.
    python tools/edge_mask_bench.py [molecules=65536] [em_steps=20] [div_molecules=2048]
Absent rows are still computed (masked rows only drop out of the per-atom sums), so a masked batch is expected to cost about what
the complete graph costs."""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def radius_mask(x, keep=0.5):
    """[B, A] mask of the pairs closer than the `keep` quantile of all distances (symmetric, about `keep` of the pairs)."""
    A = x.shape[1]
    d = np.linalg.norm(x[:, :, None] - x[:, None, :], axis=-1)
    off = ~np.eye(A, dtype=bool)
    cut = np.quantile(d[:256][:, off], keep)
    present = (d <= cut) & off[None]                      # present[b, s, d]
    return (present.astype(np.uint64) << np.arange(A, dtype=np.uint64)[None, :, None]).sum(axis=1).astype(np.uint32), float(present[:, off].mean())


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    Bd = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    import torch
    syn, W, E = ti.synthetic, ti.weights, ti.engine
    F, L, A = 128, 5, 18
    tpl = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, F, L, 25, 0), W.painn_param_spec(W.AMBIENT, F, L, 25))
    eng = E.PainnEngine(W.AMBIENT, F, L, A, *tpl, np.arange(A), flat, temp_length=100.0, precision="f16x2")
    x, cond = syn.molecule_coords(B, A, seed=0), syn.ambient_cond(B, A)
    half, frac = radius_mask(x)
    ones = np.full((B, A), (1 << A) - 1, np.uint32)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cond).cuda()
    grid = E.time_grid(0.0, 1.0, steps + 1)
    out = {"workload": f"EM rollout, {B} x {A} atoms, F={F} L={L} f16x2, {steps} steps", "radius_mask_pair_fraction": frac}
    ends = {}
    for name, m in (("no_mask", None), ("all_ones", ones), ("radius_half", half), ("no_mask_again", None)):
        eng.set_edge_mask(m)
        eng.rollout(xd, cd, E.time_grid(0.0, 1.0, 3), scheme="em", eps=0.01, seed=1, save_every=0)     # warm-up: workspace, row words
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        path, _ = eng.rollout(xd, cd, grid, scheme="em", eps=0.01, seed=1, save_every=0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[f"{name}_steps_per_s"] = B * steps / dt
        out[f"{name}_layout"] = eng.template_for(B)
        ends[name] = path[-1].cpu().numpy()
    out["all_ones_bit_identical_to_no_mask"] = bool(np.array_equal(ends["all_ones"], ends["no_mask"]))
    xs, cs = x[:Bd], cond[:Bd]
    hs, _ = radius_mask(xs)
    for name, m in (("div_no_mask", None), ("div_radius_half", hs)):
        eng.set_edge_mask(m)
        eng.drift_div(xs, 0.5, cs)
        t0 = time.perf_counter()
        for _ in range(3):
            _, div = eng.drift_div(xs, 0.5, cs)
        dt = (time.perf_counter() - t0) / 3
        out[f"{name}_molecule_evaluations_per_s"] = Bd / dt
        out[f"{name}_finite"] = bool(np.isfinite(div).all())
    eng.set_edge_mask(None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
