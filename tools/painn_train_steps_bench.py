#!/usr/bin/env python3
"""Time per step of ti_painn_train_steps against the loop of ti_painn_train_step calls it replaces, at the flagship model (F 128, L 5,
A 18, fully connected) for B in --batches.  Per batch size, in one process:
  steps      one call of --steps optimiser steps on device-resident sets and indices (ambient, standard loss)
  loop       --steps calls of PainnTrainer.step on host arrays gathered on the host, as thermo.ambient.Trainer.step drives them
  forward    one call with update = 0 against --steps calls of PainnTrainer.grad on the same host arrays
  latent     one call on a multi-T latent model (one-sided loss) with a given x0, with drawn and with aligned base samples: the
             noise kernel's share of a latent step is the difference
Wall time of the whole call or loop divided by --steps; `--repeats` timings after `--warmup`, the median and the range.  With --out
the lines go to a file (profiles/painn_train_steps_bench.txt).  --once runs one 8-step call per batch size and nothing else: the run
to put under a kernel trace.

  python tools/painn_train_steps_bench.py --out profiles/painn_train_steps_bench.txt
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


def timed(fn, warmup, repeats, per):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3 / per)
    return f"{np.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f})", float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,12")
    ap.add_argument("--shape", default="128x5x18", help="FxLxA")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--pool", type=int, default=1024, help="molecules in either resident set")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    F, L, A = (int(v) for v in a.shape.split("x"))
    W, syn = ti.weights, ti.synthetic
    src, dst, et = syn.fully_connected_template(A)
    ids = np.arange(A) % 25

    def trainer(variant):
        spec = W.painn_param_spec(variant, F, L, 25)
        flat = W.flatten_state_dict(syn.painn_state_dict(variant, F, L, 25, 0), spec).astype(np.float64)
        return ti.engine.PainnTrainer(variant, F, L, A, src, dst, et, ids, flat, lr=1e-4)

    n, K = a.pool, a.steps
    x0, x1 = syn.molecule_coords(n, A, seed=1), syn.molecule_coords(n, A, seed=2) * 1.5
    t0 = np.full(n, 1000.0, np.float32)
    t1 = (300.0 + 100.0 * (np.arange(n) % 6)).astype(np.float32)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    dx0, dx1, dt0, dt1 = dev(x0), dev(x1), dev(t0), dev(t1)
    amb, lat = trainer(W.AMBIENT), trainer(W.LATENT_MULTI)
    lines = [f"molecule trainer, ms per step: F {F} L {L} A {A} ({src.size} edges per molecule), {K} steps a call or loop, sets of {n} molecules; "
             f"median of {a.repeats} (min .. max) after {a.warmup}"]
    for B in (int(v) for v in a.batches.split(",")):
        rs = np.random.default_rng(B)
        i0, i1 = (np.stack([rs.permutation(n)[:B] for _ in range(K)]).astype(np.int64) for _ in range(2))
        di0, di1 = dev(i0), dev(i1)
        kw = dict(seed=1, draw=0)
        if a.once:
            print(B, amb.steps(dx0, dx1, dt0, dt1, di0[:8].contiguous(), di1[:8].contiguous(), **kw)[0])
            continue
        rows = [(np.ascontiguousarray(x0[i0[k]]), np.ascontiguousarray(x1[i1[k]]),
                 np.ascontiguousarray(np.stack([np.repeat(t0[i0[k]][:, None], A, 1), np.repeat(t1[i1[k]][:, None], A, 1)], -1))) for k in range(K)]
        s_txt, s_ms = timed(lambda: amb.steps(dx0, dx1, dt0, dt1, di0, di1, **kw), a.warmup, a.repeats, K)
        l_txt, l_ms = timed(lambda: [amb.step(*rows[k], seed=1, draw=k) for k in range(K)], a.warmup, a.repeats, K)
        f_txt, _ = timed(lambda: amb.steps(dx0, dx1, dt0, dt1, di0, di1, update=False, **kw), a.warmup, a.repeats, K)
        g_txt, _ = timed(lambda: [amb.grad(*rows[k], seed=1, draw=k) for k in range(K)], a.warmup, a.repeats, K)
        lk = dict(kind="one_sided", t_distr="beta_2_1", **kw)
        given, g_ms = timed(lambda: lat.steps(dx0, dx1, None, dt1, di0, di1, **lk), a.warmup, a.repeats, K)
        drawn, d_ms = timed(lambda: lat.steps(None, dx1, None, dt1, None, di1, noise="drawn", **lk), a.warmup, a.repeats, K)
        align, a_ms = timed(lambda: lat.steps(None, dx1, None, dt1, None, di1, noise="aligned", **lk), a.warmup, a.repeats, K)
        lines += [f"B {B}: steps {s_txt} ms, loop of step calls {l_txt} ms (ratio {l_ms / s_ms:.3f}); forward only {f_txt} ms, loop of grad calls {g_txt} ms",
                  f"B {B}: latent step with given x0 {given} ms, drawn {drawn} ms, aligned {align} ms: the aligned noise is {100.0 * (a_ms - g_ms) / a_ms:+.2f} % "
                  f"of a latent step (drawn {100.0 * (d_ms - g_ms) / d_ms:+.2f} %)"]
        print("\n".join(lines[-2:]), flush=True)
    if a.out and not a.once:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
