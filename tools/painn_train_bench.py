#!/usr/bin/env python3
"""Time of ti_painn_train_grad and ti_painn_train_step at the flagship model (F 128, L 5, A 18, fully connected, ambient, standard
loss) for B in --batches: device-resident inputs, wall time of a call (its one synchronisation inside), `--repeats` calls after
`--warmup`; prints the median and the range and the workspace of the call, and with --out writes them to a file
(profiles/painn_train_bench.txt).  A batch above the default workspace budget is replaced by the largest one that fits.
--once runs one step per batch and nothing else: the run to put under a kernel trace.

  python tools/painn_train_bench.py --out profiles/painn_train_bench.txt
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ti = importlib.import_module("thermodynamic-interpolation_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64,512")
    ap.add_argument("--shape", default="128x5x18", help="FxLxA")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--graphs", action="store_true", help="also time `step` with a full table of per-molecule graphs in force "
                    "(ti_painn_train_set_graphs: the masked twins on rows none of which is dead; profiles/painn_train_graphs_bench.txt)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    F, L, A = (int(v) for v in a.shape.split("x"))
    W, syn = ti.weights, ti.synthetic
    spec = W.painn_param_spec(W.AMBIENT, F, L, 25)
    flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, F, L, 25, 0), spec).astype(np.float64)
    src, dst, et = syn.fully_connected_template(A)
    tr = ti.engine.PainnTrainer(W.AMBIENT, F, L, A, src, dst, et, np.arange(A) % 25, flat, lr=1e-4)
    lines = [f"molecule trainer, ms per call: F {F} L {L} A {A} ({src.size} edges per molecule, {flat.size} parameters), ambient, standard loss, "
             f"batch centring, device-resident inputs, median of {a.repeats} calls (min .. max) after {a.warmup}"]
    for B in (int(v) for v in a.batches.split(",")):
        while tr.workspace_bytes(B) > ti._lib.PAINN_TRAIN_DEFAULT_WORKSPACE:
            B -= 1
        dev = lambda v: torch.from_numpy(v).cuda()
        x0, x1 = dev(syn.molecule_coords(B, A, seed=1)), dev(syn.molecule_coords(B, A, seed=2) * 1.5)
        cond = dev(syn.ambient_cond(B, A))
        if a.once:
            print(B, tr.step(x0, x1, cond, seed=1, draw=0))
            continue
        res = {}
        calls = [("grad", lambda k: tr.grad(x0, x1, cond, seed=1, draw=k)), ("step", lambda k: tr.step(x0, x1, cond, seed=1, draw=k))]
        if a.graphs:
            calls.append(("step, full table", lambda k: tr.step(x0, x1, cond, seed=1, draw=k)))
        for name, fn in calls:
            tr.set_graphs(np.full(B, A, np.int32)) if name.endswith("table") else tr.set_graphs()
            for k in range(a.warmup):
                fn(k)
            ms = []
            for k in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(a.warmup + k)
                ms.append((time.perf_counter() - t0) * 1e3)
            res[name] = f"{name} {np.median(ms):.2f} ({min(ms):.2f} .. {max(ms):.2f}) ms"
        tr.set_graphs()
        lines.append(f"B {B}: {', '.join(res.values())}; workspace {tr.workspace_bytes(B) / 2 ** 30:.2f} GiB, {2 * B * src.size} edge rows")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out and not a.once:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
