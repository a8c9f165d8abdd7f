#!/usr/bin/env python
"""Generate tests/golden/obs_geometry.npz: the reference's internal-coordinate functions and effective sample size on seeded inputs.

    python tests/golden/make_golden_obs.py --reference /path/to/thermodynamic-interpolation

Only imports from the reference checkout (mdqm9/analysis/utils/mol_geometry.py: compute_distance, compute_angle, compute_torsion;
mdqm9/analysis/utils/ess.py: calc_ESS) and records what they return; the fixture holds seeded fp32 coordinates (B = 7 molecules of
A = 9 atoms), the index tuples, the reference's values (computed in fp32, as the reference's analysis does) and calc_ESS of seeded
weights.  Molecules 0..2 carry a torsion near 0, near +pi and near -pi on atoms (0, 1, 2, 3); molecule 3 an angle near pi on atoms
(4, 5, 6).  No exactly collinear triple enters a torsion (the reference divides by zero there); every recorded value is finite."""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def coordinates():
    rs = np.random.RandomState(20240607)
    x = rs.standard_normal((7, 9, 3)) * 1.5
    # planar four-atom chains with a small out-of-plane shift of the last atom: torsion ~ 0 (cis), ~ +pi and ~ -pi (trans)
    for b, (y3, lift) in enumerate([(1.1, 0.012), (-1.1, 0.011), (-1.1, -0.009)]):
        x[b, 0], x[b, 1], x[b, 2], x[b, 3] = [1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.3, y3, lift]
    # a nearly straight triple: angle ~ pi - 0.25
    x[3, 4], x[3, 5] = [2.0, 0.0, 0.0], [0.5, 0.0, 0.0]
    x[3, 6] = [0.5 - 1.3 * np.cos(0.25), 1.3 * np.sin(0.25), 0.0]
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TI_REFERENCE"), required=os.environ.get("TI_REFERENCE") is None)
    ap.add_argument("--out", default=os.path.join(HERE, "obs_geometry.npz"))
    args = ap.parse_args()
    import torch
    utils = os.path.join(args.reference, "mdqm9", "analysis", "utils")
    geo = _load("ref_mol_geometry", os.path.join(utils, "mol_geometry.py"))
    ess = _load("ref_ess", os.path.join(utils, "ess.py"))

    x = coordinates()
    dist_idx = np.array([(0, 1), (1, 2), (2, 3), (0, 8), (4, 6), (7, 5)], np.int32)
    angle_idx = np.array([(0, 1, 2), (1, 2, 3), (4, 5, 6), (8, 0, 7), (3, 6, 2)], np.int32)
    torsion_idx = np.array([(0, 1, 2, 3), (1, 2, 3, 4), (5, 6, 7, 8), (8, 3, 0, 6), (3, 2, 1, 0)], np.int32)
    for t in torsion_idx:                      # no collinear triple inside a torsion
        for tri in (t[:3], t[1:]):
            a, b = x[:, tri[0]] - x[:, tri[1]], x[:, tri[2]] - x[:, tri[1]]
            assert (np.linalg.norm(np.cross(a, b), axis=-1) > 1e-3).all(), t
    xt = torch.from_numpy(x)
    at = lambda i: xt[:, int(i)]
    dist = np.stack([geo.compute_distance(at(i), at(j)).numpy() for i, j in dist_idx], axis=1)
    angle = np.stack([geo.compute_angle(at(i), at(j), at(k)).numpy() for i, j, k in angle_idx], axis=1)
    torsion = np.stack([geo.compute_torsion(at(i), at(j), at(k), at(l)).numpy() for i, j, k, l in torsion_idx], axis=1)
    assert all(np.isfinite(v).all() for v in (dist, angle, torsion))
    assert abs(torsion[0, 0]) < 0.05 and torsion[1, 0] > np.pi - 0.05 and torsion[2, 0] < -np.pi + 0.05, torsion[:3, 0]
    assert np.pi - 0.3 < angle[3, 2] < np.pi - 0.2, angle[3, 2]

    rs = np.random.RandomState(7)
    logw = rs.standard_normal(500) * 3.0
    weights = np.exp(logw)
    np.savez(args.out, x=x, dist_idx=dist_idx, angle_idx=angle_idx, torsion_idx=torsion_idx, dist=dist.astype(np.float32),
             angle=angle.astype(np.float32), torsion=torsion.astype(np.float32), weights=weights, ess=np.float64(ess.calc_ESS(weights)))
    sys.path.insert(0, os.path.dirname(HERE))
    import obs_numpy as on
    p = lambda idx: [x[:, i] for i in idx]
    print("max |reference - fp64 restatement|:",
          max(np.abs(dist[:, k] - on.distance(*p(t))).max() for k, t in enumerate(dist_idx)),
          max(np.abs(angle[:, k] - on.angle(*p(t))).max() for k, t in enumerate(angle_idx)),
          max(np.abs(torsion[:, k] - on.torsion(*p(t))).max() for k, t in enumerate(torsion_idx)))
    print("torsions (0,1,2,3):", torsion[:3, 0], "angle:", angle[3, 2], "ess:", ess.calc_ESS(weights))


if __name__ == "__main__":
    main()
