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
