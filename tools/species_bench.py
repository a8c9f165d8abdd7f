#!/usr/bin/env python3
"""Mixed-species batches against one call per species: 64 species x 64 molecules, A from 9 to 25 atoms (complete graphs), F = 128,
L = 5, f16x2, 20 Euler steps on device-resident buffers.
    python tools/species_bench.py [species=64] [molecules_per_species=64] [steps=20] [repeats=7]
"mixed": one handle whose template is the largest species, ti_painn_set_molecules, one rollout of all species x molecules.
"per_species": one handle per species (created before the clock starts), one rollout each, one after the other: the sum is what a
user without mixed batches pays.  Every timed region follows a warm-up rollout of the same call and ends with a device synchronise;
the figure is the median of `repeats` runs, with the spread beside it.  Pad rows are computed like absent rows, so the mixed call
does the arithmetic of species x molecules of the LARGEST species; what it saves is launches and latency-bound small batches.
Prints one JSON line."""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def timed(fn, sync, repeats):
    fn()
    sync()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    import torch
    syn, W, E = ti.synthetic, ti.weights, ti.engine
    F, L = 128, 5
    sizes = np.round(np.linspace(9, 25, S)).astype(np.int32)
    A = int(sizes.max())
    flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, F, L, 25, 0), W.painn_param_spec(W.AMBIENT, F, L, 25))
    grid = E.time_grid(0.0, 1.0, steps + 1)
    sync = torch.cuda.synchronize

    def handle(a):
        return E.PainnEngine(W.AMBIENT, F, L, a, *syn.fully_connected_template(a), np.arange(a), flat, temp_length=100.0, precision="f16x2")

    xs = [syn.molecule_coords(M, int(a), seed=k) for k, a in enumerate(sizes)]
    cs = [syn.ambient_cond(M, int(a)) for a in sizes]
    x = np.zeros((S * M, A, 3), np.float32)
    c = np.zeros((S * M, A, 2), np.float32)
    for k, a in enumerate(sizes):
        x[k * M:(k + 1) * M, :a], c[k * M:(k + 1) * M, :a] = xs[k], cs[k]
    n_atoms = np.repeat(sizes, M)

    mixed = handle(A)
    mixed.set_molecules(n_atoms)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    ends = {}

    def run_mixed():
        ends["mixed"] = mixed.rollout(xd, cd, grid, scheme="euler", save_every=0)[0]

    t_mixed = timed(run_mixed, sync, repeats)
    layout = mixed.template_for(S * M)

    t0 = time.perf_counter()
    per = [handle(int(a)) for a in sizes]
    t_create = time.perf_counter() - t0
    xds = [torch.from_numpy(v).cuda() for v in xs]
    cds = [torch.from_numpy(v).cuda() for v in cs]

    def run_per_species():
        ends["per"] = [h.rollout(xv, cv, grid, scheme="euler", save_every=0)[0] for h, xv, cv in zip(per, xds, cds)]

    t_per = timed(run_per_species, sync, repeats)
    end = ends["mixed"][-1].cpu().numpy()
    worst = max(float(np.abs(end[k * M:(k + 1) * M, :a] - ends["per"][k][-1].cpu().numpy()).max()) for k, a in enumerate(sizes))
    print(json.dumps({
        "workload": f"Euler rollout, {S} species x {M} molecules, A {int(sizes.min())}..{A}, F={F} L={L} f16x2, {steps} steps",
        "mixed_call_s": t_mixed[0], "mixed_call_min_max_s": t_mixed[1:], "mixed_layout": layout,
        "per_species_calls_sum_s": t_per[0], "per_species_min_max_s": t_per[1:], "per_species_layout": per[0].template_for(M),
        "per_species_handle_creation_s_not_in_the_sum": t_create, "per_species_over_mixed": t_per[0] / t_mixed[0],
        "max_abs_end_state_difference": worst, "repeats": repeats}))


if __name__ == "__main__":
    main()
