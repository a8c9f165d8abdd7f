"""Drop-in mirror of the reference ambient sampling API (thermo/ambient) on top of libti_hip.so.

  cPaiNN             <- /root/reference/mdqm9/thermo/ambient/models/cpainn.py:10-115
  MoleculeIntegrator <- /root/reference/mdqm9/thermo/ambient/integrators.py:8-68
"""
from __future__ import annotations

from .. import weights as _W
from . import interpolants, losses  # noqa: F401  (the reference's thermo.ambient.interpolants / .losses)
from ._molecule import DEFAULT_TEMPS, MoleculeIntegratorBase, MoleculeTrainerBase, ODEWrapperBase, PaiNNShell


class cPaiNN(PaiNNShell):
    VARIANT, ATOM_KEY, COND_KEYS = _W.AMBIENT, "atoms", ("T0", "T1")

    def __init__(self, n_features: int = 32, embedding_layers: int = 2, score_layers: int = 5, n_types=25, temp_length=10, time_length=10,
                 temperatures=DEFAULT_TEMPS):
        self.embedding_layers = embedding_layers          # unused by the reference as well (dead constructor argument)
        self._init(n_features, score_layers, n_types, temp_length, time_length, temperatures)


class ODEWrapper(ODEWrapperBase):
    """thermo/ambient/models/ode_wrapper.py:6-113"""
    DIV_SCALE = 1e-2


class MoleculeIntegrator(MoleculeIntegratorBase):
    """rollout(batch) -> (xts [n_saved, N, 3], dlogp * 1e2, n_fevals, batch.batch)   (integrators.py:68)"""
    SCALE_DLOGP = 1e2
    DIV_SCALE = 1e-2

    def rollout(self, batch, traj_offset: int = 0):
        xts, dlogp, nfe = self._rollout(batch, traj_offset)
        return xts, dlogp, nfe, batch.batch


class Trainer(MoleculeTrainerBase):
    """Trains an ambient cPaiNN on StandardVelocityLoss (train_ambient.py:124-149): step(batch0, batch1) is one optimiser step on the
    pair of batches the reference's loader yields (batch0.x at T0, batch1.x at T1; fields as losses.forward reads them)."""
    BETA_NAME = "beta_half"

    def step(self, batch0, batch1, *, t=None, z=None, seed=0, draw=0, traj_offset=0, center=None) -> float:
        """One optimiser step -> the batch's mean loss (NaN where the step was skipped)"""
        return self._step(batch0, batch0.x, batch1.x, (batch0.T, batch1.T), t, z, seed, draw, traj_offset, center)

    def loss(self, batch0, batch1, *, t=None, z=None, seed=0, draw=0, traj_offset=0, center=None) -> float:
        """The mean loss at the current weights by the trainer's own forward pass; nothing is updated"""
        return self._loss(batch0, batch0.x, batch1.x, (batch0.T, batch1.T), t, z, seed, draw, traj_offset, center)

    def fit(self, x0, temps0, x1, temps1, batch_size, n_steps, seed, **kw):
        """n_steps optimiser steps in one device call on the resident sets (x0 [n0, A, 3] at temps0 [n0], x1 [n1, A, 3] at temps1 [n1]):
        MoleculeTrainerBase.fit.  -> (mean loss of every step, the number of skipped steps)"""
        return MoleculeTrainerBase.fit(self, x0, x1, temps0, temps1, batch_size, n_steps, seed, **kw)

    def evaluate(self, x0, temps0, x1, temps1, batch_size, n_steps, seed, **kw):
        """The loss of the same minibatches at the current weights, nothing updated -> [n_steps]"""
        return MoleculeTrainerBase.evaluate(self, x0, x1, temps0, temps1, batch_size, n_steps, seed, **kw)
