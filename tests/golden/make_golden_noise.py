#!/usr/bin/env python3
"""Generate tests/golden/painn_noise_align.npz: the aligned base samples of the latent data set (the reference's
mdqm9_latent.py:84-105) with scipy.spatial.transform.Rotation.align_vectors as the yardstick of the rotation.

Two groups of molecules, A = 3 (three centred points are coplanar: the correlation matrix has rank 2) and A = 9.  The draws are the
library's own, N(seed, traj_offset + b, draw, 3 a + c) by the host oracle, centred in fp64 (tests/painn_noise_numpy.py).  Of the
A = 9 group, molecule 0 has x1 = x0 (the identity), molecule 1 has x1 = the mirror image of x0 (the unconstrained SVD has determinant
-1 and the correction decides); every other x1 is a centred random molecule.  Per group g in ("a3", "a9"):
    x1_g [B, A, 3] float32, x0_g [B, A, 3] float64 (drawn and centred), rot_g [B, 3, 3] float64 (scipy), aligned_g [B, A, 3] float64,
    gap_g [B] the relative gap of the two largest eigenvalues of Horn's matrix; and seed, traj_offset_g, draw.
Every molecule kept has gap >= 1e-3: the rotation is then well conditioned, and two fp64 evaluations of it agree far below an fp32 ulp.
    python tests/golden/make_golden_noise.py
"""
import os
import sys

import numpy as np
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import painn_noise_numpy as pn  # noqa: E402

SEED, DRAW = 20240607, 5
GROUPS = {"a3": (3, 4, 100), "a9": (9, 12, (1 << 33) + 7)}      # A, B, traj_offset (one above 2^32: the high counter word)
MIN_GAP = 1e-3


def main():
    out = dict(seed=np.int64(SEED), draw=np.int64(DRAW))
    rs = np.random.RandomState(11)
    for g, (A, B, off) in GROUPS.items():
        xc = pn.centre(pn.draw(SEED, off, DRAW, B, A))
        x1 = rs.standard_normal((B, A, 3))
        x1 = (x1 - x1.mean(axis=1, keepdims=True)).astype(np.float32)
        if A == 9:
            x1[0] = xc[0].astype(np.float32)
            x1[1] = (xc[1] * np.array([-1.0, 1.0, 1.0])).astype(np.float32)
        R = np.empty((B, 3, 3))
        gap = np.empty(B)
        for b in range(B):
            R[b] = Rotation.align_vectors(x1[b].astype(np.float64), xc[b])[0].as_matrix()
            gap[b] = pn.horn_gap(x1[b].astype(np.float64), xc[b])
            assert gap[b] >= MIN_GAP, (g, b, gap[b])
            assert abs(np.linalg.det(R[b]) - 1.0) < 1e-12
        if A == 9:
            assert np.abs(R[0] - np.eye(3)).max() < 1e-6
            K = x1[1].astype(np.float64).T @ xc[1]
            U, _, Vt = np.linalg.svd(K)
            assert np.linalg.det(U @ Vt) < 0.0                     # the mirror molecule: the correction decides
        out.update({f"x1_{g}": x1, f"x0_{g}": xc, f"rot_{g}": R, f"aligned_{g}": np.einsum("bij,baj->bai", R, xc), f"gap_{g}": gap,
                    f"traj_offset_{g}": np.int64(off)})
        print(g, "gaps", np.array2string(gap, precision=3))
    np.savez(os.path.join(HERE, "painn_noise_align.npz"), **out)


if __name__ == "__main__":
    main()
