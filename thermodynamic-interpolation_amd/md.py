"""Langevin dynamics under a force field on the GPU (include/ti_hip.h ti_obs_ff_langevin): the sampler that produces the
multi-temperature training sets the loaders of data.py read, from an OpenMM System export and one geometry, without OpenMM.

``LangevinSampler`` keeps the fp64 state (positions in nm, velocities in nm/ps) across calls and advances the global step index
itself, so that a run made of many calls is the run of one call bit for bit: the noise is keyed by (seed, replica id, global step).
``ReplicaExchangeSampler`` adds temperature ladders with exchanges of neighbouring rungs (ti_obs_ff_remd), keyed by (seed, ladder id,
attempt index) in the same way.
"""
from __future__ import annotations

import numpy as np


class LangevinSampler:
    """Replicas of one species under ``ff`` on ``engine`` (a PainnEngine for the species; the force field is set on it here).

    to_nm: nm per model length unit (frames are returned in model units, x0 is taken in them); dt in ps, friction in 1/ps, seed the
    Philox key.  ``start(x0, T, ids=None)`` places the replicas -- x0 [B, A, 3] model units, T [B] kelvin -- and draws their
    velocities from N(0, R T / m); ``equilibrate(n)`` advances n steps without output; ``sample(n_frames, stride)`` returns
    (frames [B, n_frames, A, 3] float32 centred model units, epot, ekin [B, n_frames] float64 kJ/mol)."""

    def __init__(self, engine, ff, to_nm, dt, friction, seed, steps_per_launch=0):
        if not (np.isfinite(to_nm) and to_nm > 0):
            raise ValueError(f"to_nm must be finite and > 0, got {to_nm!r}")
        self.engine, self.ff, self.to_nm = engine, ff, float(to_nm)
        self.dt, self.friction, self.seed, self.steps_per_launch = float(dt), float(friction), int(seed), int(steps_per_launch)
        engine.set_forcefield(ff)
        self.pos = self.vel = self.T = self.ids = None
        self.step = 0

    def start(self, x0, T, ids=None):
        x0 = np.asarray(x0)
        self.pos = np.ascontiguousarray(x0, np.float64) * self.to_nm
        B = self.pos.shape[0]
        self.T = np.full(B, float(T), np.float32) if np.shape(T) == () else np.ascontiguousarray(T, np.float32)
        self.ids = np.arange(B, dtype=np.int64) if ids is None else np.ascontiguousarray(ids, np.int64)
        self.step = 0
        # zero steps: the call only draws the velocities (components 3A.. at step index 0, which no noise draw uses)
        self.pos, self.vel, _, _, _ = self._run(0, 0, draw=True)
        return self

    def _run(self, n_steps, stride, draw=False):
        if self.pos is None:
            raise RuntimeError("LangevinSampler.start(x0, T) first")
        out = self.engine.langevin(self.pos, None if draw else self.vel, self.T, self.dt, self.friction, n_steps, stride=stride,
                                   step_offset=self.step, seed=self.seed, ids=self.ids, to_nm=self.to_nm, draw_velocities=draw,
                                   steps_per_launch=self.steps_per_launch)
        self.step += int(n_steps)
        return out

    def equilibrate(self, n):
        self.pos, self.vel, _, _, _ = self._run(int(n), 0)
        return self

    def sample(self, n_frames, stride):
        n_frames, stride = int(n_frames), int(stride)
        if n_frames < 1 or stride < 1:
            raise ValueError("n_frames and stride must be >= 1")
        self.pos, self.vel, frames, epot, ekin = self._run(n_frames * stride, stride)
        return frames, epot, ekin


def round_trips(walkers):
    """Bottom -> top -> bottom passages per ladder.  walkers [n, n_ladders, K] (or [n, K]: one ladder): entry [t, l, k] is the rung at
    which the configuration at rung k of ladder l after attempt t started (the identity before the first).  A configuration completes
    a round trip when, having been at rung 0, it reaches rung K - 1 and then rung 0 again; the count of a ladder sums over its K
    configurations -> [n_ladders] int64."""
    w = np.asarray(walkers)
    w = w[:, None] if w.ndim == 2 else w
    if w.ndim != 3:
        raise ValueError(f"walkers must be [n, n_ladders, K] or [n, K], got {w.shape}")
    n, L, K = w.shape
    trips = np.zeros(L, np.int64)
    state = np.zeros((L, K), np.int8)                           # per configuration: 0 not yet at the bottom, 1 left the bottom, 2 reached the top
    state[:, 0] = 1                                             # the identity start: configuration 0 is at rung 0
    for t in range(n):
        bottom, top = w[t, :, 0], w[t, :, K - 1]
        rows = np.arange(L)
        trips += state[rows, bottom] == 2
        state[rows, bottom] = 1
        up = state[rows, top] == 1
        state[rows[up], top[up]] = 2
    return trips


class ReplicaExchangeSampler(LangevinSampler):
    """n_ladders temperature ladders of one species (include/ti_hip.h ti_obs_ff_remd): LangevinSampler with Metropolis exchanges of
    neighbouring rungs after every ``exchange_every``-th step of the run.  ``start(x0, ladder_T, n_ladders, ids=None)`` places the
    rows ladder-major -- x0 [n_ladders * K, A, 3] model units, ladder_T [K] kelvin ascending, row l * K + k rung k of ladder l, ids
    [n_ladders * K] the replica ids of the noise, ladder_ids [n_ladders] the keys of the exchange draws; ``equilibrate`` and
    ``sample`` as there, a frame at the step of an attempt showing the state before it.  Kept across calls: ``counts`` [n_ladders,
    K - 1, 2] int64 (attempts, acceptances of each neighbouring pair), ``acceptance`` [K - 1] (over ladders; NaN before an attempt),
    ``walker`` [n_ladders * K] and ``walkers`` [n_attempts, n_ladders, K], the labels after every attempt so far (round_trips reads
    them)."""

    def __init__(self, engine, ff, to_nm, dt, friction, seed, exchange_every, steps_per_launch=0):
        super().__init__(engine, ff, to_nm, dt, friction, seed, steps_per_launch)
        if int(exchange_every) < 1:
            raise ValueError(f"exchange_every must be >= 1, got {exchange_every!r}")
        self.exchange_every = int(exchange_every)
        self.K = self.ladder_ids = self.walker = self.walkers = self.counts = None

    def start(self, x0, ladder_T, n_ladders, ids=None, ladder_ids=None):
        ladder_T = np.ascontiguousarray(ladder_T, np.float32).reshape(-1)
        K, L = len(ladder_T), int(n_ladders)
        if K < 2 or L < 1 or np.shape(x0)[0] != K * L:
            raise ValueError(f"a ladder needs >= 2 rungs and x0 one geometry per row: {L} ladders of {K} rungs, x0 {np.shape(x0)}")
        self.K = K
        self.ladder_ids = np.arange(L, dtype=np.int64) if ladder_ids is None else np.ascontiguousarray(ladder_ids, np.int64)
        self.walker = np.tile(np.arange(K, dtype=np.int32), L)
        self.walkers = np.zeros((0, L, K), np.int32)
        self.counts = np.zeros((L, K - 1, 2), np.int64)
        return super().start(x0, np.tile(ladder_T, L), ids)

    @property
    def acceptance(self):
        c = self.counts.sum(axis=0).astype(np.float64)
        return np.where(c[:, 0] > 0, c[:, 1] / np.maximum(c[:, 0], 1.0), np.nan)

    def _run(self, n_steps, stride, draw=False):
        if self.pos is None:
            raise RuntimeError("ReplicaExchangeSampler.start(x0, ladder_T, n_ladders) first")
        out = self.engine.remd(self.pos, None if draw else self.vel, self.T, self.K, self.exchange_every, self.dt, self.friction, n_steps,
                               stride=stride, step_offset=self.step, seed=self.seed, ids=self.ids, ladder_ids=self.ladder_ids,
                               walker=self.walker, to_nm=self.to_nm, draw_velocities=draw, steps_per_launch=self.steps_per_launch)
        self.step += int(n_steps)
        self.walker = np.asarray(out[5], np.int32)
        self.walkers = np.concatenate([self.walkers, np.asarray(out[6], np.int32).reshape(-1, len(self.ladder_ids), self.K)])
        self.counts = self.counts + np.asarray(out[7], np.int64)
        return out[:5]
