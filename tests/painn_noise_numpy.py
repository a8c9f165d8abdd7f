"""numpy restatement of the latent base samples (include/ti_hip.h ti_painn_train_noise): the Philox normal of the host oracle,
per-molecule centring with the fp64 sum in atom order, and the proper rotation onto x1 by Kabsch (numpy.linalg.svd with the
determinant correction)."""
import numpy as np


def draw(seed, traj_offset, draw_index, B, A):
    """x0 [B, A, 3] float32: oracle.normal(seed, traj_offset + b, draw, 3 a + c), bit for bit the kernel's draw"""
    from oracle import oracle
    return np.asarray([[[oracle.normal(seed, traj_offset + b, draw_index, 3 * a + c) for c in range(3)] for a in range(A)] for b in range(B)],
                      np.float32)


def centre(x):
    """x [B, A, 3] float32 -> float64: each molecule minus its mean over the atoms, the sum taken in atom order from +0.0 (a loop: numpy's
    own sum is pairwise), divided by A, subtracted in fp64.  Not rounded."""
    x = np.asarray(x, np.float32).astype(np.float64)
    s = np.zeros((x.shape[0], 3))
    for a in range(x.shape[1]):
        s = s + x[:, a]
    return x - (s / float(x.shape[1]))[:, None, :]


def kabsch(x1, x0):
    """The proper rotation R [3, 3] (det +1) that minimises sum_a |x1_a - R x0_a|^2, x1 and x0 [A, 3] float64:
    K = sum_a x1_a x0_a^T = U S V^T, R = U diag(1, 1, det(U V^T)) V^T."""
    K = np.asarray(x1, np.float64).T @ np.asarray(x0, np.float64)
    U, _, Vt = np.linalg.svd(K)
    d = 1.0 if np.linalg.det(U @ Vt) >= 0.0 else -1.0
    return U @ np.diag([1.0, 1.0, d]) @ Vt


def horn_gap(x1, x0):
    """(lambda_1 - lambda_2) / lambda_1 of Horn's 4 x 4 quaternion matrix of K = sum_a x1_a x0_a^T: the conditioning of the rotation"""
    S = np.asarray(x0, np.float64).T @ np.asarray(x1, np.float64)          # S[i][j] = sum_a x0_a[i] x1_a[j]
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = S
    N = np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                  [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                  [zx - xz, xy + yx, -xx + yy - zz, yz + zy],
                  [xy - yx, zx + xz, yz + zy, -xx - yy + zz]])
    w = np.linalg.eigvalsh(N)
    return float((w[-1] - w[-2]) / w[-1])


def noise(seed, traj_offset, draw_index, x1, aligned, A=None, B=None):
    """-> (x0 [B, A, 3] float32, R [B, 3, 3] float64 | None, the centred draws in float64) as ti_painn_train_noise returns them"""
    if x1 is not None:
        B, A = x1.shape[:2]
    xc = centre(draw(seed, traj_offset, draw_index, B, A))
    if not aligned:
        return xc.astype(np.float32), None, xc
    R = np.stack([kabsch(np.asarray(x1[b], np.float32).astype(np.float64), xc[b]) for b in range(B)])
    return np.einsum("bij,baj->bai", R, xc).astype(np.float32), R, xc
