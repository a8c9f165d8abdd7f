#!/usr/bin/env python3
"""Time per optimiser step of the adw trainer (ti_adw_train_steps): `--steps` indexed steps in one call, host arrays in, wall time of
the call divided by the steps (the upload of the sets and the one synchronisation are inside), repeated `--repeats` times after a
warm-up call; prints the median and the spread and, with --out, writes them to a file (profiles/adw_train_step_bench.txt).

  python tools/adw_train_bench.py --out profiles/adw_train_step_bench.txt
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

# launches of one step: gather 4, draw 1, interpolate 1, inputs 2, forward 3 + (L + 1), loss rows 1, sums 2 + 2, output gradient 1,
# net backward 3 (L + 1) - 1, embedding gradient 1, beta_embed backward 8, combine 1, optimiser 1, counters 1
launches = lambda L: 4 + 1 + 1 + 2 + 3 + (L + 1) + 1 + 4 + 1 + 3 * (L + 1) - 1 + 1 + 8 + 1 + 1 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x5x512,64x3x512,256x5x4096", help="comma-separated HxLxB")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=8192, help="rows of either resident set")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = [f"adw trainer, us per optimiser step: {a.steps} indexed steps per call, median of {a.repeats} calls (min .. max), sets of {a.rows} rows, d = 1"]
    rs = np.random.RandomState(0)
    for shape in a.shapes.split(","):
        H, L, B = (int(v) for v in shape.split("x"))
        W = ti.weights
        flat = W.flatten_state_dict(ti.synthetic.adw_state_dict(H, L, 0), W.adw_param_spec(H, L), dtype=np.float64)
        tr = ti.engine.AdwTrainer(H, L, flat)
        x0, x1 = rs.standard_normal(a.rows).astype(np.float32), (1.5 * rs.standard_normal(a.rows) + 1.0).astype(np.float32)
        b0, b1 = np.full(a.rows, 1.0, np.float32), np.full(a.rows, 1.25, np.float32)
        i0, i1 = rs.randint(0, a.rows, (a.steps, B)), rs.randint(0, a.rows, (a.steps, B))
        tr.steps(x0, x1, b0, b1, i0[:5], i1[:5], a=0.9)
        us = []
        for r in range(a.repeats):
            t0 = time.perf_counter()
            loss, skipped = tr.steps(x0, x1, b0, b1, i0, i1, a=0.9, draw=5 + r * a.steps)
            us.append((time.perf_counter() - t0) / a.steps * 1e6)
        n = launches(L)
        lines.append(f"H {H} L {L} B {B}: {np.median(us):.1f} ({min(us):.1f} .. {max(us):.1f}) us per step, {n} launches, "
                     f"{np.median(us) / n:.2f} us per launch; skipped {skipped}")
        tr.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
