#!/usr/bin/env python3
"""Z-matrix calls of the synthetic A = 18 species on the GPU: ti_obs_zmat, ti_obs_zmat_xyz (with log|det J| and the validity mask) and
ti_obs_hist_cols at the headline batches with every array in device memory; ti_obs_hist_cols over the K = 48 internal coordinates
against the 48 ti_obs_hist calls it replaces (the same entry point as before, one column per call, same box); and the numpy
restatement (tests/zmat_numpy.py) on 4 096 of the same molecules on the host for scale.
    timeout -k 10 300 python tools/zmat_bench.py [batches=65536,1048576] [repeats=7]
Every timed call ends in the library's stream synchronise; the median of the repeats after a warm-up call is reported."""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def timed(fn, reps):
    fn()                                                                          # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                                      # returns after the handle's stream is synchronised
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3, min(times) * 1e3, max(times) * 1e3


def main():
    batches = [int(b) for b in (sys.argv[1] if len(sys.argv) > 1 else "65536,1048576").split(",")]
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 7, 5)
    import torch
    import zmat_numpy as zn
    ti = importlib.import_module("thermodynamic-interpolation_amd")
    syn, W, E = ti.synthetic, ti.weights, ti.engine
    A, n_host, bins = 18, 4096, 64
    rs = np.random.RandomState(0)
    bonds = np.array([[i, rs.randint(0, i)] for i in range(1, A)])
    zm = ti.zmatrix.ZMatrix.from_bonds(bonds, A)
    tpl = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, 32, 1, 25, 0), W.painn_param_spec(W.AMBIENT, 32, 1, 25))
    eng = E.PainnEngine(W.AMBIENT, 32, 1, A, *tpl, np.arange(A), flat, temp_length=100.0)
    z_host = np.zeros((n_host, A - 1, 3), np.float32)
    z_host[:, :, 0] = rs.uniform(0.9, 1.6, (n_host, A - 1))
    z_host[:, 1:, 1] = rs.uniform(1.2, 2.6, (n_host, A - 2))
    z_host[:, 2:, 2] = rs.uniform(-3.1, 3.1, (n_host, A - 3))
    t0 = time.perf_counter()
    x64, ld64, _, _ = zn.deconstruct(z_host, zm.order, zm.ref)
    host_xyz = time.perf_counter() - t0
    x_host = x64.astype(np.float32)
    t0 = time.perf_counter()
    z64 = zn.construct(x_host, zm.order, zm.ref)
    host_z = time.perf_counter() - t0
    print(f"synthetic species: A = {A}, a random tree, K = {3 * A - 6} internal coordinates")
    print(f"host, numpy restatement, {n_host} molecules: construct {host_z * 1e3:.1f} ms = {n_host / host_z:.3e} molecules/s, "
          f"deconstruct {host_xyz * 1e3:.1f} ms = {n_host / host_xyz:.3e} molecules/s")
    results = []
    for B in batches:
        tile = lambda a: torch.from_numpy(a).cuda().repeat((B + n_host - 1) // n_host, 1, 1)[:B].contiguous()
        x, z = tile(x_host), tile(z_host)
        logw = torch.from_numpy((np.random.RandomState(1).standard_normal(B) * 2).astype(np.float32)).cuda()
        keep = torch.from_numpy(ti.zmatrix.iqr_keep(logw, 100.0)).cuda()
        out = {}
        t_z = timed(lambda: out.__setitem__("z", eng.zmatrix(x, zm)), reps)
        t_x = timed(lambda: out.__setitem__("x", eng.zmatrix_xyz(z, zm, logdet=True, valid=True)), reps)
        err_z = float(np.abs(out["z"][:n_host].cpu().numpy() - z64).max())
        err_x = float(np.abs(out["x"][0][:n_host].cpu().numpy() - x64).max())
        # the 48 internal coordinates as one [B, 48] array: what a user held as ti_obs_cv descriptors before
        cols = torch.from_numpy(ti.zmatrix.marginal_columns(A)).cuda()
        v = out["z"].reshape(B, -1)[:, cols].contiguous()
        K = int(v.shape[1])
        lo = np.where(np.arange(K) < A - 1, 0.0, np.where(np.arange(K) < 2 * A - 3, 0.0, -np.pi))
        hi = np.where(np.arange(K) < A - 1, 4.0, np.pi)
        t_c = timed(lambda: out.__setitem__("c", eng.hist_cols(v, logw, None, bins, lo, hi)), reps)
        t_k = timed(lambda: eng.hist_cols(v, logw, keep, bins, lo, hi), reps)
        t_1 = timed(lambda: out.__setitem__("h", [eng.weighted_histogram(v[:, c], logw, bins, (lo[c], hi[c])) for c in range(K)]), reps)
        same = all((out["c"][0][c].view(np.uint64) == out["h"][c][0].view(np.uint64)).all() for c in range(K))
        t_m = timed(lambda: ti.observables.zmatrix_marginals(out["z"], logw, keep, bins, engine=eng), reps)
        for name, t in (("ti_obs_zmat", t_z), ("ti_obs_zmat_xyz (+ logdet, valid)", t_x), (f"ti_obs_hist_cols, K = {K}", t_c),
                        (f"ti_obs_hist_cols, K = {K}, keep", t_k), (f"{K} x ti_obs_hist", t_1), ("zmatrix_marginals (K = 51 columns of z, keep)", t_m)):
            print(f"GPU, device memory, {B} molecules, {name}: median of {reps} calls {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f}) = {B / t[0] * 1e3:.3e} molecules/s")
        print(f"  hist_cols against the {K} calls it replaces: {t_1[0] / t_c[0]:.1f} x faster, every column bit-identical: {same}; "
              f"zmat {B / t_z[0] * 1e3 / (n_host / host_z):.0f} x the host, zmat_xyz {B / t_x[0] * 1e3 / (n_host / host_xyz):.0f} x the host; "
              f"against the host's values: z {err_z:.1e}, x {err_x:.1e}")
        results.append(dict(molecules=B, zmat_ms=t_z[0], zmat_xyz_ms=t_x[0], hist_cols_ms=t_c[0], hist_cols_keep_ms=t_k[0], hist_x48_ms=t_1[0],
                            marginals_ms=t_m[0], bit_identical=bool(same), max_err_z=err_z, max_err_x=err_x))
        del x, z, v, logw, keep, out
    print(json.dumps({"workload": f"Z-matrix calls, synthetic A = {A} species, device memory", "host_construct_molecules_per_s": n_host / host_z,
                      "host_deconstruct_molecules_per_s": n_host / host_xyz, "results": results}))


if __name__ == "__main__":
    main()
