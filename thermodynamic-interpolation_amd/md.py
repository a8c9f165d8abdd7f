"""Langevin dynamics under a force field on the GPU (include/ti_hip.h ti_obs_ff_langevin): the sampler that produces the
multi-temperature training sets the loaders of data.py read, from an OpenMM System export and one geometry, without OpenMM.

``LangevinSampler`` keeps the fp64 state (positions in nm, velocities in nm/ps) across calls and advances the global step index
itself, so that a run made of many calls is the run of one call bit for bit: the noise is keyed by (seed, replica id, global step).
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
