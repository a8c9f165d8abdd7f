#!/usr/bin/env python3
"""Wall time of ti_obs_bg_logw (the Boltzmann-generator log-weights) at B = 65 536 molecules of m = 54 components with every input in
device memory: the median of 7 calls after 2 warm-up calls, written to profiles/bg_bench.txt.  A record only: the kernel reads
B (4 m + 16) bytes = 15 MB and writes 12 B per molecule, nothing is promised about it and there is no earlier figure to compare with.
    timeout -k 10 120 python tools/bg_bench.py [B=65536] [m=54] [out=profiles/bg_bench.txt]
Every timed call ends in the library's stream synchronise."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

WARMUP, REPEATS = 2, 7


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    m = int(sys.argv[2]) if len(sys.argv) > 2 else 54
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "bg_bench.txt")
    import torch
    import bg_numpy as bgn
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    eng = ti.observables._service_engine(0)
    rs = np.random.RandomState(0)
    z = rs.standard_normal((B, m)).astype(np.float32)
    u1, nb, nt = 5.0 * rs.standard_normal(B), (3.0 * rs.standard_normal(B)).astype(np.float32), (3.0 * rs.standard_normal(B)).astype(np.float32)
    dz, du, db, dt_ = (torch.from_numpy(a).cuda() for a in (z, u1, nb, nt))
    for _ in range(WARMUP):
        lw, lp = eng.bg_logw(dz, du, db, dt_, logpz=True)
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        lw, lp = eng.bg_logw(dz, du, db, dt_, logpz=True)                     # returns after the handle's stream is synchronised
        times.append(time.perf_counter() - t0)
    n = min(B, 4096)
    ref_lp, ref_lw = bgn.bg_logw(z[:n], u1[:n], nb[:n], nt[:n])
    exact = bool(np.array_equal(lp[:n].cpu().numpy(), ref_lp) and np.array_equal(lw[:n].cpu().numpy(), ref_lw))
    med = float(np.median(times))
    read = B * (4 * m + 16)
    lines = [f"ti_obs_bg_logw, B = {B}, m = {m}, device memory, both outputs ({torch.cuda.get_device_name(0)})",
             f"median of {REPEATS} calls after {WARMUP} warm-up calls: {med * 1e6:.1f} us (min {min(times) * 1e6:.1f}, max {max(times) * 1e6:.1f}), "
             f"allocation of the two outputs and the stream synchronise included",
             f"bytes read {read} ({read / med / 1e9:.1f} GB/s at the median), {B / med:.3e} molecules/s",
             f"first {n} molecules equal the numpy restatement bit for bit: {exact}"]
    print("\n".join(lines))
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
