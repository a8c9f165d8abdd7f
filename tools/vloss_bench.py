#!/usr/bin/env python3
"""Velocity loss (ti_painn_vloss / ti_adw_vloss) on the GPU, everything in device memory: the time of one velocity_loss call at the
headline shape (65 536 molecules x 18 atoms, F 128, L 5, f16x2, ambient) and at adw with 262 144 rows (H 256, 5 layers, f32), and
beside it -- in the same process, alternated call by call -- the plain drift on the 2B states at per-molecule times, which is what
the call evaluates in its middle.  The difference is what the two new stages (interpolate, reduce) add.  Stage one is also timed
alone (interpolate: its kernels plus the device-to-device copies of t, z and xt it returns); what is left of the difference is
the reduce stage with the copies of the losses.  Bytes are computed from the shapes (below) and set against 6.3 TB/s.
    timeout -k 10 600 python tools/vloss_bench.py [repeats=7] [out=profiles/vloss_bench.txt]
Every timed call ends in the library's stream synchronise; medians of the repeats after one warm-up round are reported.  The stage
times are CALL times, not kernel times: per-kernel times of the new kernels are not measured by this tool."""
import importlib
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM = 6.3e12


def med(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), min(ts), max(ts)


def report(out, tag, B, m, n_cond, centred, loss, drift, interp, reps):
    """m floats per row; n_cond conditioning floats per row.  Bytes from the shapes: stage one reads x0, x1 (8 m B), t, writes z (4 m B)
    and xt (8 m B) -- and with centring writes and re-reads the fp64 states (2 x 16 m B) and reads them once more for the column
    sums (16 m B); its call also copies t, z, xt out (2 x (4 + 12 m) B).  Reduce reads x0, x1, z, b (20 m B), t and writes 8 B per row."""
    s1 = (8 * m + 4 + 4 * m + 8 * m + (48 * m if centred else 0)) * B
    s1_call = s1 + 2 * (4 + 12 * m) * B
    s3 = (20 * m + 4 + 8) * B + 2 * 8 * B
    added = loss[0] - drift[0]
    red = added - interp[0]
    line = lambda *a: out.append(" ".join(str(x) for x in a))
    line(f"== {tag}: B = {B}, {m} floats per row, medians of {reps} alternated calls")
    line(f"velocity_loss           {loss[0] * 1e3:9.3f} ms  (min {loss[1] * 1e3:.3f}, max {loss[2] * 1e3:.3f})  = {B / loss[0]:.3e} rows/s")
    line(f"drift on 2B, per-row t  {drift[0] * 1e3:9.3f} ms  (min {drift[1] * 1e3:.3f}, max {drift[2] * 1e3:.3f})")
    line(f"added by the new stages {added * 1e3:9.3f} ms  = {100 * added / loss[0]:.2f} % of the call")
    line(f"interpolate call alone  {interp[0] * 1e3:9.3f} ms  (min {interp[1] * 1e3:.3f}, max {interp[2] * 1e3:.3f}); {s1_call / 1e6:.1f} MB with its output copies "
         f"({s1 / 1e6:.1f} MB in its kernels) -> {s1_call / interp[0] / 1e12:.3f} TB/s = {100 * s1_call / interp[0] / HBM:.1f} % of 6.3 TB/s")
    if red > 0:
        line(f"reduce, by difference   {red * 1e3:9.3f} ms; {s3 / 1e6:.1f} MB -> {s3 / red / 1e12:.3f} TB/s = {100 * s3 / red / HBM:.1f} % of 6.3 TB/s "
             f"(a difference of medians: indicative only)")
    else:
        line(f"reduce, by difference   not resolved (the difference of the medians is {red * 1e3:.3f} ms)")


def main():
    reps = max(int(sys.argv[1]) if len(sys.argv) > 1 else 7, 5)
    dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "vloss_bench.txt")
    import torch
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    syn, W, E = ti.synthetic, ti.weights, ti.engine
    out = [f"tools/vloss_bench.py on {socket.gethostname()}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    # ---- molecules, the headline shape
    B, A, F, L = 65536, 18, 128, 5
    tpl = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, F, L, 25, 0), W.painn_param_spec(W.AMBIENT, F, L, 25))
    eng = E.PainnEngine(W.AMBIENT, F, L, A, *tpl, np.arange(A), flat, temp_length=100.0, precision="f16x2")
    base = 4096
    rep = lambda a: dev(a).repeat(B // base, *([1] * (a.ndim - 1))).contiguous()
    x0, x1, cond = rep(syn.molecule_coords(base, A, seed=1)), rep(syn.molecule_coords(base, A, seed=2)), rep(syn.ambient_cond(base, A))
    kw = dict(gamma="brownian", a=0.9, center="batch", seed=1)
    r = eng.velocity_loss(x0, x1, cond, returns=("t", "xt"), **kw)              # warm-up, and the states the drift leg evaluates
    xt2, t2, c2 = r["xt"].reshape(2 * B, A, 3).contiguous(), r["t"].repeat(2).contiguous(), cond.repeat(2, 1, 1).contiguous()
    ob = torch.empty_like(xt2)
    eng.drift(xt2, t2, c2, out=ob)
    eng.interpolate(x0, x1, **kw)
    tl, td, ti_ = [], [], []
    for _ in range(reps):                                                       # alternated: one of each per round
        tl.append(med(lambda: eng.velocity_loss(x0, x1, cond, **kw), 1)[0])
        td.append(med(lambda: eng.drift(xt2, t2, c2, out=ob), 1)[0])
        ti_.append(med(lambda: eng.interpolate(x0, x1, **kw), 1)[0])
    st = lambda v: (float(np.median(v)), min(v), max(v))
    out.append(f"mean loss of the warm-up call {r['mean']:.6f} (synthetic weights)")
    report(out, "ambient, A 18, F 128, L 5, f16x2, centre BATCH, brownian a 0.9, drawn t and z", B, 3 * A, 2 * A, True, st(tl), st(td), st(ti_), reps)
    del x0, x1, cond, xt2, t2, c2, ob, r
    eng.close()

    # ---- adw, 262 144 rows
    B, H, nl = 262144, 256, 5
    flat = W.flatten_state_dict(syn.adw_state_dict(H, nl, 0), W.adw_param_spec(H, nl), dtype=np.float64)
    ea = E.AdwEngine(H, nl, flat)
    x0, x1 = dev(syn.adw_boltzmann(B, 1.0, seed=1).astype(np.float32)), dev(syn.adw_boltzmann(B, 1.25, seed=2).astype(np.float32))
    b0, b1 = torch.full((B,), 1.0, device=x0.device), torch.full((B,), 1.25, device=x0.device)
    kw = dict(a=0.9, seed=1)
    r = ea.velocity_loss(x0, x1, b0, b1, returns=("t", "xt"), **kw)
    xt2, t2, b02, b12 = r["xt"].reshape(2 * B).contiguous(), r["t"].repeat(2).contiguous(), b0.repeat(2).contiguous(), b1.repeat(2).contiguous()
    ob = torch.empty_like(xt2)
    ea.drift(xt2, t2, b02, b12, out=ob)
    ea.interpolate(x0, x1, **kw)
    tl, td, ti_ = [], [], []
    for _ in range(reps):
        tl.append(med(lambda: ea.velocity_loss(x0, x1, b0, b1, **kw), 1)[0])
        td.append(med(lambda: ea.drift(xt2, t2, b02, b12, out=ob), 1)[0])
        ti_.append(med(lambda: ea.interpolate(x0, x1, **kw), 1)[0])
    report(out, "adw, H 256, 5 layers, f32, brownian a 0.9, drawn t and z", B, 1, 2, False, st(tl), st(td), st(ti_), reps)
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
