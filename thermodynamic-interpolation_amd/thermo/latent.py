"""Drop-in mirror of the reference latent sampling API (thermo/latent) on top of libti_hip.so.

  cPaiNN             <- /root/reference/mdqm9/thermo/latent/models/cpainn.py:10-108
  MoleculeIntegrator <- /root/reference/mdqm9/thermo/latent/integrators.py:8-89
"""
from __future__ import annotations

from .. import weights as _W
from . import interpolants, losses  # noqa: F401  (the reference's thermo.latent.interpolants / .losses)
from ._molecule import DEFAULT_TEMPS, MoleculeIntegratorBase, MoleculeTrainerBase, ODEWrapperBase, PaiNNShell


class cPaiNN(PaiNNShell):
    ATOM_KEY = "atom_number"

    def __init__(self, n_features: int = 32, score_layers: int = 5, n_types=25, time_length=10, temp_length=10, temperatures=DEFAULT_TEMPS):
        # one temperature feature T, or none when the model knows a single temperature (cpainn.py:43-72)
        multi = len(temperatures) > 1
        self.VARIANT = _W.LATENT_MULTI if multi else _W.LATENT_SINGLE
        self.COND_KEYS = ("T",) if multi else ()
        self._init(n_features, score_layers, n_types, temp_length, time_length, temperatures)


class ODEWrapper(ODEWrapperBase):
    """thermo/latent/models/ode_wrapper.py:6-113"""
    DIV_SCALE = 1.0


class MoleculeIntegrator(MoleculeIntegratorBase):
    """rollout(batch) -> (xts [n_saved, N, 3], dlogp, batch.batch)   (integrators.py:89; no 1e2 scaling in latent)"""
    SCALE_DLOGP = 1.0

    def rollout(self, batch, traj_offset: int = 0):
        xts, dlogp, self.n_fevals = self._rollout(batch, traj_offset)
        return xts, dlogp, batch.batch

    def log_prob(self, batch):
        """log p_model(x) [B] float64 of the conformations in batch.x0 (where rollout reads its start state), the model being this
        map applied to N(0, I) noise.  Build-defined: the reference has no such function; -log_prob on held-out MD frames is a
        Boltzmann generator's usual validation number.  One rollout with return_dlogp=True on this integrator's own method, step
        count, tolerances and divergence settings carries x back along the same field, (b, -div b) on the grid from `end` down to
        `start`, to z_end with the end-state dlogp d; then, in fp64,
            log_prob = observables.log_prior(z_end) - d.
        The sign follows from one identity: a forward run from z0 to x1 with end-state neg_dlogp has log p_model(x1) =
        log_prior(z0) + neg_dlogp (the second state integrates -div b), and on the way back the same pair over negative steps
        integrates +div b, so d = -neg_dlogp up to the solver's error.  reverse_ode=True is NOT this inverse: as in the reference
        (ode_wrapper.py:49, integrators.py:40-43) it negates b AND descends the grid, which pushes x forward a second time -- on
        the CPU oracle its z_end misses z0 by O(1) and the composed density misses the identity by 1.4 where this rollout meets it to
        9e-5 (div_latent_multi, heun, 9 grid points).  As in ``observables.bg_logw`` the prior is the full 3A-dimensional normal.
        One species per call.  Lives where batch.x0 lives."""
        import numpy as np
        from .. import observables as _obs
        from . import _common as C
        from ._molecule import split_species_batch
        sb = split_species_batch(batch, self.b.ATOM_KEY)
        if sb.n_atoms is not None:
            raise ValueError("log_prob takes one species per call (the prior's dimension is 3A)")
        saved = self.return_dlogp, self.reverse_ode, self.start, self.end
        self.return_dlogp, self.reverse_ode, self.start, self.end = True, False, self.end, self.start
        try:
            xts, dlogp, self.n_fevals = self._rollout(batch)
        finally:
            self.return_dlogp, self.reverse_ode, self.start, self.end = saved
        z_end = C.as_f32(xts[-1], (sb.B, 3 * sb.A))
        d = dlogp[-1]
        lp = _obs.log_prior(z_end, engine=self.b.engine_of(sb))
        if C.is_cuda(z_end):
            import torch
            return lp - d.to(torch.float64)
        return C.like(lp - C.to_numpy(d).astype(np.float64), batch.x0)


class Trainer(MoleculeTrainerBase):
    """Trains a latent cPaiNN on OneSidedVelocityLoss (train_latent.py): step(batch) is one optimiser step on a batch with the noise
    in batch.x0 and the data in batch.x1 (fields as losses.forward reads them)."""
    BETA_NAME = "beta_2_1"

    def _conds(self, batch):
        return tuple(getattr(batch, k) for k in self.b.COND_KEYS)

    def step(self, batch, *, t=None, z=None, seed=0, draw=0, traj_offset=0, center=None) -> float:
        """One optimiser step -> the batch's mean loss (NaN where the step was skipped)"""
        return self._step(batch, batch.x0, batch.x1, self._conds(batch), t, z, seed, draw, traj_offset, center)

    def loss(self, batch, *, t=None, z=None, seed=0, draw=0, traj_offset=0, center=None) -> float:
        """The mean loss at the current weights by the trainer's own forward pass; nothing is updated"""
        return self._loss(batch, batch.x0, batch.x1, self._conds(batch), t, z, seed, draw, traj_offset, center)

    @staticmethod
    def _noise(noise):
        return (None, noise) if isinstance(noise, str) else (noise, "given")

    def fit(self, x1, temps1, batch_size, n_steps, seed, *, noise="drawn", **kw):
        """n_steps optimiser steps in one device call on the resident set x1 [n, A, 3] (temps1 [n], None for a single-temperature
        model).  noise: "drawn" or "aligned" (the base samples of mdqm9_latent.py:84-105 drawn on the device for every minibatch, the
        latter rotated onto x1), or a given x0 [n0, A, 3].  -> (mean loss of every step, the number of skipped steps)"""
        x0, noise = self._noise(noise)
        return MoleculeTrainerBase.fit(self, x0, x1, None, temps1, batch_size, n_steps, seed, noise=noise, **kw)

    def evaluate(self, x1, temps1, batch_size, n_steps, seed, *, noise="drawn", **kw):
        """The loss of the same minibatches at the current weights, nothing updated -> [n_steps]"""
        x0, noise = self._noise(noise)
        return MoleculeTrainerBase.evaluate(self, x0, x1, None, temps1, batch_size, n_steps, seed, noise=noise, **kw)
