"""numpy restatement of ti_obs_bg_logw (include/ti_hip.h; csrc/obs_bg_kernels.hip): the lane order, the butterfly and the two
expressions in fp64, operation for operation, so that the GPU's outputs can be compared bit for bit.

    lane l:  s_l = sum of (double)z[b, c]^2 over c = l, l + 64, ... in that order, from +0.0
    wave:    for o in 32, 16, 8, 4, 2, 1: s_l += s_(l xor o)          (every lane ends with the same bits; lane 0 is read)
    logpz = -(0.5 * S) - (m * HALF_LOG_2PI)                            (the product rounded before the subtraction)
    logw  = (float32) -(((u1 + logpz) + nd_bg) + nd_ti)                (an absent term is +0.0)
"""
import numpy as np

HALF_LOG_2PI = 0.9189385332046727


def lane_sums(z):
    """[B, 64] float64: the per-lane sums of squares of z [B, m] float32"""
    z = np.asarray(z, np.float32)
    B, m = z.shape
    v = z.astype(np.float64)
    s = np.zeros((B, 64), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for c0 in range(0, m, 64):
            n = min(64, m - c0)
            s[:, :n] = s[:, :n] + v[:, c0:c0 + n] * v[:, c0:c0 + n]
    return s


def wave_sum(s):
    """the butterfly with offsets 32 .. 1 over axis 1 of s [B, 64]; every column ends with the same bits"""
    s = np.array(s, np.float64)
    lanes = np.arange(64)
    with np.errstate(over="ignore", invalid="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
    return s


def log_prior(z):
    """[B] float64 of z [B, m] float32"""
    z = np.asarray(z, np.float32)
    z = z.reshape(z.shape[0], -1)
    S = wave_sum(lane_sums(z))[:, 0]
    with np.errstate(over="ignore", invalid="ignore"):
        return -(0.5 * S) - (np.float64(z.shape[1]) * np.float64(HALF_LOG_2PI))


def bg_logw(z, u1=None, nd_bg=None, nd_ti=None):
    """(logpz [B] float64, logw [B] float32)"""
    lp = log_prior(z)
    B = lp.shape[0]
    term = lambda a: np.zeros(B, np.float64) if a is None else np.asarray(a).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return lp, (-(((term(u1) + lp) + term(nd_bg)) + term(nd_ti))).astype(np.float32)
