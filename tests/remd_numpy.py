"""numpy restatement of replica exchange as the library computes it (include/ti_hip.h ti_obs_ff_remd), written from the header: the
Langevin segments are ff_forces_numpy.langevin, the energies those of its force pass, the exchange draw vloss_numpy.philox4x32_10
with the fp32 uniform and the host libm's logf restated below.  `replay` re-derives every decision of a run from given energies: the
oracle of the exact decision tests of tests/test_gpu_remd.py.  Nothing here runs on a GPU or needs the package."""
import numpy as np

import ff_numpy as fn
import ff_forces_numpy as ffn
import vloss_numpy as vn

REMD_DOMAIN = 0x52454D44
REMD_MAX_RUNGS = 64

_INVC = [float.fromhex(s) for s in (
    "0x1.661ec79f8f3bep+0", "0x1.571ed4aaf883dp+0", "0x1.49539f0f010bp+0", "0x1.3c995b0b80385p+0", "0x1.30d190c8864a5p+0",
    "0x1.25e227b0b8eap+0", "0x1.1bb4a4a1a343fp+0", "0x1.12358f08ae5bap+0", "0x1.0953f419900a7p+0", "0x1p+0", "0x1.e608cfd9a47acp-1",
    "0x1.ca4b31f026aap-1", "0x1.b2036576afce6p-1", "0x1.9c2d163a1aa2dp-1", "0x1.886e6037841edp-1", "0x1.767dcf5534862p-1")]
_LOGC = [float.fromhex(s) for s in (
    "-0x1.57bf7808caadep-2", "-0x1.2bef0a7c06ddbp-2", "-0x1.01eae7f513a67p-2", "-0x1.b31d8a68224e9p-3", "-0x1.6574f0ac07758p-3",
    "-0x1.1aa2bc79c81p-3", "-0x1.a4e76ce8c0e5ep-4", "-0x1.1973c5a611cccp-4", "-0x1.252f438e10c1ep-5", "0x0p+0", "0x1.aa5aa5df25984p-5",
    "0x1.c5e53aa362eb4p-4", "0x1.526e57720db08p-3", "0x1.bc2860d22477p-3", "0x1.1058bc8a07ee1p-2", "0x1.4043057b6ee09p-2")]


def uniform24(word):
    """((word >> 8) + 0.5) 2^-24 in fp32: exact, never 0 or 1"""
    return ((np.asarray(word, np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def host_logf(x):
    """glibc's logf (the Arm Optimized Routines' algorithm) of normal fp32 x > 0, in fp64 operations in the libm's order -> fp32"""
    x = np.asarray(x, np.float32)
    ix = x.view(np.uint32).astype(np.int64)
    tmp = (ix - 0x3f330000) & 0xFFFFFFFF
    i = (tmp >> 19) % 16
    k = ((tmp ^ 0x80000000) - 0x80000000) >> 23                 # the arithmetic shift of the signed word
    iz = (ix - (tmp & 0xff800000)) & 0xFFFFFFFF
    z = iz.astype(np.uint32).view(np.float32).astype(np.float64)
    r = z * np.asarray(_INVC)[i] - 1.0
    y0 = np.asarray(_LOGC)[i] + k.astype(np.float64) * float.fromhex("0x1.62e42fefa39efp-1")
    r2 = r * r
    y = float.fromhex("0x1.5575b0be00b6ap-2") * r + float.fromhex("-0x1.ffffef20a4123p-2")
    y = float.fromhex("-0x1.00ea348b88334p-2") * r2 + y
    y = y * r2 + (y0 + r)
    return np.where(ix == 0x3f800000, np.float32(0), y.astype(np.float32))


def pairs(n, K):
    """the lower rungs k of the pairs (k, k + 1) of attempt n"""
    return list(range(n % 2, K - 1, 2))


def counter(ladder_id, n, k):
    """the four counter words of the draw of pair (k, k + 1) of attempt n (the word taken is k & 3)"""
    lid = int(ladder_id) & 0xFFFFFFFFFFFFFFFF
    return [lid & 0xFFFFFFFF, lid >> 32, int(n) & 0xFFFFFFFF, (REMD_DOMAIN + (k >> 2)) & 0xFFFFFFFF]


def draw_logu(seed, ladder_id, n, k):
    """(double)logf(u) of the pair (k, k + 1) of attempt n of the ladder"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    o = vn.philox4x32_10(np.asarray([counter(ladder_id, n, k)], np.uint64), (seed & 0xFFFFFFFF, seed >> 32))
    return float(host_logf(uniform24(o[0, k & 3])))


def decide(E, T, seed, ladder_id, n, dead=None, ft=np.float64):
    """One attempt of one ladder: E [K] the energies of its rungs, T [K] fp32 kelvin -> {k: (accept, delta, logu)} over the pairs of
    attempt n.  delta = (beta_k - beta_k1) (E_k - E_k1) in `ft`, beta = 1 / (R (double)T); accept iff both energies are finite,
    neither rung is in `dead`, and delta >= 0 or logu < delta."""
    E, T = np.asarray(E, ft), np.asarray(T, np.float32).astype(ft)
    out = {}
    for k in pairs(n, len(E)):
        with np.errstate(invalid="ignore", over="ignore"):
            delta = (ft(1) / (ft(fn.R_GAS) * T[k]) - ft(1) / (ft(fn.R_GAS) * T[k + 1])) * (E[k] - E[k + 1])
        logu = draw_logu(seed, ladder_id, n, k)
        ok = bool(np.isfinite(E[k]) and np.isfinite(E[k + 1])) and not (dead is not None and (dead[k] or dead[k + 1]))
        out[k] = (ok and bool(delta >= 0 or ft(logu) < delta), float(delta), logu)
    return out


def replay(epot, T, K, seed, ladder_ids, attempts, walker=None):
    """Every decision of a run from its energies.  epot [B, n_attempts]: column j the energies of the rows right before attempt
    attempts[j] (a run with stride == exchange_every returns exactly these as out_epot); T [B]; rows ladder-major.  Returns (walkers
    [n_attempts, B] after each attempt, counts [n_ladders, K - 1, 2], accepted {(j, ladder, k): bool}, margins: the |logu - delta| of
    every decision)."""
    epot = np.asarray(epot, np.float64)
    B = epot.shape[0]
    L = B // K
    w = (np.arange(B) % K).astype(np.int32) if walker is None else np.array(walker, np.int32)
    ladder_ids = np.arange(L) if ladder_ids is None else ladder_ids
    hist, counts, accepted, margins = [], np.zeros((L, K - 1, 2), np.int64), {}, []
    for j, n in enumerate(attempts):
        for l in range(L):
            rows = slice(l * K, (l + 1) * K)
            for k, (acc, delta, logu) in decide(epot[rows, j], T[rows], seed, ladder_ids[l], n).items():
                counts[l, k, 0] += 1
                counts[l, k, 1] += acc
                accepted[(j, l, k)] = acc
                margins.append(abs(logu - delta))
                if acc:
                    w[l * K + k], w[l * K + k + 1] = w[l * K + k + 1], w[l * K + k]
        hist.append(w.copy())
    return np.array(hist, np.int32).reshape(len(attempts), B), counts, accepted, np.array(margins)


def remd(pos, vel, T, ids, ladder_ids, K, exchange_every, ff, masses, dt, friction, n_steps, stride=0, step_offset=0, seed=0, to_nm=1.0,
         draw=False, walker=None, normal=ffn.oracle_normal, ft=np.float64, flip_delta=False, rescale=True, stored=False):
    """ti_obs_ff_remd as the header states it -> (pos, vel, frames, epot, ekin, walker, walkers [n_attempts, B], counts, margins).  The
    segments between two cuts -- at every frame and at every attempt -- are ff_forces_numpy.langevin (chaining repeats it bit for
    bit); an attempt follows global step count g whenever g % exchange_every == 0, after the frame due there.  An accepted pair
    exchanges positions and velocities, the velocity at the positions' time v + (dt / 2) f / m rescaled by sqrt(T_new / T_old).
    flip_delta, rescale=False (no rescale) and stored=True (the stored velocity rescaled as it is): the mutations the physics test
    catches (profiles/remd_mutations.txt)."""
    pos = np.array(pos, ft)
    B, A = pos.shape[:2]
    half, mass = ft(np.float64(dt)) * ft(0.5), np.asarray(masses, np.float64).astype(ft)[None, :, None]
    L = B // K
    pairs_table = fn.pair_table(ff, A)
    ladder_ids = np.arange(L) if ladder_ids is None else ladder_ids
    Tft = np.asarray(T, np.float32).astype(ft)
    w = (np.arange(B) % K).astype(np.int32) if walker is None else np.array(walker, np.int32)
    kw = dict(ff=ff, masses=masses, dt=dt, friction=friction, seed=seed, to_nm=to_nm, normal=normal, ft=ft, pairs=pairs_table)
    if draw:
        vel = ffn.draw_velocities(T, ids, masses, seed, step_offset, normal, ft)
    vel = np.array(vel, ft)
    frames, epot, ekin, hist, margins = [], [], [], [], []
    counts = np.zeros((L, K - 1, 2), np.int64)
    done = 0
    while done < n_steps:
        g = step_offset + done
        to_frame = stride - done % stride if stride > 0 else n_steps
        n = min(n_steps - done, to_frame, (g // exchange_every + 1) * exchange_every - g)
        due = stride > 0 and (done + n) % stride == 0
        pos, vel, f, e, k_ = ffn.langevin(pos, vel, T, ids, n_steps=n, stride=n if due else 0, step_offset=g, **kw)
        done += n
        if due:
            frames.append(f[:, 0]); epot.append(e[:, 0]); ekin.append(k_[:, 0])
        if (g + n) % exchange_every == 0:
            att = (g + n) // exchange_every
            F, _, E, _ = ffn.forces_nm(pos, ff, pairs_table)
            kick = half * F / mass                               # (dt / 2) f / m: what the stored velocity lags behind the positions
            for l in range(L):
                rows = slice(l * K, (l + 1) * K)
                Eu = -E[rows] if flip_delta else E[rows]
                for k, (acc, delta, logu) in decide(Eu, T[rows], seed, ladder_ids[l], att, ft=ft).items():
                    a, b = l * K + k, l * K + k + 1
                    counts[l, k, 0] += 1
                    counts[l, k, 1] += acc
                    margins.append(abs(logu - delta))
                    if acc:
                        up, down = (np.sqrt(Tft[b] / Tft[a]), np.sqrt(Tft[a] / Tft[b])) if rescale else (ft(1), ft(1))
                        pos[[a, b]] = pos[[b, a]]
                        if stored:
                            vel[a], vel[b] = vel[b] * down, vel[a] * up
                        else:
                            vel[a], vel[b] = (vel[b] + kick[b]) * down - kick[b], (vel[a] + kick[a]) * up - kick[a]
                        w[a], w[b] = w[b], w[a]
            hist.append(w.copy())
    nf = len(frames)
    stack = lambda v, shape, dtype: np.stack(v, axis=1) if nf else np.zeros(shape, dtype)
    return (pos, vel, stack(frames, (B, 0, A, 3), np.float32), stack(epot, (B, 0), ft), stack(ekin, (B, 0), ft), w,
            np.array(hist, np.int32).reshape(len(hist), B), counts, np.array(margins))
