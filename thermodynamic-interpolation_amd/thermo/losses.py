"""Mirror of the reference velocity losses (mdqm9/thermo/{ambient,latent}/losses.py, adw/thermo/losses.py) on top of libti_hip.so
(ti_painn_vloss / ti_adw_vloss): forward evaluation only -- the number that says how good a checkpoint is in the terms it was trained
in.  The gradients of the adw forms live in the trainer (thermo.adw.Trainer, engine.AdwTrainer: ti_adw_train_*); the molecule
forms have none.

  StandardVelocityLoss(interpolant, t_distr="uniform")   forward(batch0, batch1, b)             ambient
                                                         forward(b, x0s, x1s, beta0s, beta1s)   adw
  OneSidedVelocityLoss(interpolant, t_distr="uniform")   forward(batch, b)                      latent (batch.x0 is the noise, batch.x1 the data)
                                                         forward(b, x0s, x1s, beta0s, beta1s)   adw

forward returns the mean as a Python float (the reference's loss_val.item()); `.last` holds the call's dict: loss (per molecule /
row, float64), mean, tbins ([n, 2]: sum and count per bin of t, or None), t, and z for the standard loss.
Optional keywords of every form: t= (one per molecule, or per node), z= (like x0), seed=, draw=, traj_offset= (the Philox counter of
the drawn t and z: the draws follow the reference's distributions, not torch's random streams), center= ('batch': the reference's
mean over the atom rows of the call, the default for molecules; 'molecule'; 'none'), tbins=.
t_distr "beta" is Beta(1/2, 1/2) for the ambient and adw forms and Beta(2, 1) for the latent one, as in the reference.
"""
from __future__ import annotations

import numpy as np

from . import _common as C
from ._molecule import split_graph_batch
from .interpolants import BaseInterpolant


def _molecule_t(t, B, A):
    """t given per molecule [B] or per node [N] / [N, 1] -> [B] float32 (None stays None)"""
    if t is None:
        return None
    tn = C.to_numpy(t, np.float32).reshape(-1)
    if tn.size == B:
        return np.ascontiguousarray(tn)
    if tn.size != B * A:
        raise ValueError(f"t must hold one value per molecule ({B}) or per node ({B * A}), got {tn.size}")
    per = tn.reshape(B, A)
    if np.any(per != per[:, :1]):
        raise ValueError("t must be constant within each molecule")
    return np.ascontiguousarray(per[:, 0])


class BaseVelocityLoss:
    """Base class of the velocity losses; subclasses fix the kind the interpolant must have."""
    KIND = None

    def __init__(self, interpolant: BaseInterpolant, t_distr="uniform") -> None:
        assert t_distr in ("uniform", "beta"), f"t_distr must be 'uniform' or 'beta', got {t_distr!r}"
        if getattr(interpolant, "kind", None) != self.KIND:
            raise TypeError(f"{type(self).__name__} needs a {'LinearInterpolant' if self.KIND == 'standard' else 'OneSidedLinearInterpolant'}")
        self.interpolant = interpolant
        self.t_distr = t_distr
        self.last = None

    def _kw(self, beta_name, t, seed, draw, traj_offset, tbins):
        ip = self.interpolant
        return dict(kind=self.KIND, gamma=ip.gamma_name, a=ip.a_param, t=t, t_distr="uniform" if self.t_distr == "uniform" else beta_name,
                    seed=seed, draw=draw, traj_offset=traj_offset, tbins=tbins, returns=("t", "z") if self.KIND == "standard" else ("t",))

    def forward(self, *args, t=None, z=None, seed=0, draw=0, traj_offset=0, center=None, tbins=0):
        if len(args) == 5:
            res = self._forward_adw(*args, t=t, z=z, seed=seed, draw=draw, traj_offset=traj_offset, center=center, tbins=tbins)
        elif len(args) == 3 and self.KIND == "standard":
            batch0, batch1, b = args
            res = self._forward_molecules(b, batch0, batch0.x, batch1.x, (batch0.T, batch1.T), "beta_half", t, z, seed, draw, traj_offset, center, tbins)
        elif len(args) == 2 and self.KIND == "one_sided":
            batch, b = args
            conds = tuple(getattr(batch, k) for k in b.COND_KEYS)
            res = self._forward_molecules(b, batch, batch.x0, batch.x1, conds, "beta_2_1", t, z, seed, draw, traj_offset, center, tbins)
        else:
            raise TypeError("forward takes (batch0, batch1, b) [standard, ambient], (batch, b) [one-sided, latent] or (b, x0s, x1s, beta0s, beta1s) [adw]")
        self.last = res
        return float(res["mean"])

    __call__ = forward

    def _forward_molecules(self, b, batch, x0, x1, conds, beta_name, t, z, seed, draw, traj_offset, center, tbins):
        B, A, src, dst, ety, ids, mask = split_graph_batch(batch, b.ATOM_KEY)
        eng = b.engine_with_mask(A, src, dst, ety, ids, mask)
        if len(conds) != eng.ncond:
            raise ValueError(f"this model takes {eng.ncond} conditioning value(s) per node, the batch form gives {len(conds)}")
        gpu = C.is_cuda(x0)
        x0, x1 = C.as_f32(x0, (B, A, 3)), C.as_f32(x1, (B, A, 3))
        cond = None
        if conds:
            if gpu:
                import torch
                cond = torch.stack([c.detach().to(x0.device, torch.float32).reshape(B, A) for c in conds], dim=-1).contiguous()
            else:
                cond = np.ascontiguousarray(np.stack([C.to_numpy(c).astype(np.float32).reshape(B, A) for c in conds], axis=-1))
        tv, zv = _molecule_t(t, B, A), (None if z is None else C.as_f32(z, (B, A, 3)))
        if gpu:
            import torch
            tv = None if tv is None else torch.from_numpy(tv).to(x0.device)
            zv = None if zv is None else (zv if C.is_cuda(zv) else torch.from_numpy(zv).to(x0.device))
        elif zv is not None and C.is_cuda(zv):
            zv = C.to_numpy(zv, np.float32)
        return eng.velocity_loss(x0, x1, cond, center=center or "batch", z=zv, **self._kw(beta_name, tv, seed, draw, traj_offset, tbins))

    def _forward_adw(self, b, x0s, x1s, beta0s, beta1s, *, t, z, seed, draw, traj_offset, center, tbins):
        if center not in (None, "none"):
            raise ValueError("the adw losses are not centred (center='none')")
        eng = b.engine()
        d = eng.dim
        shape = (-1,) if d == 1 else (-1, d)
        x0 = np.ascontiguousarray(C.to_numpy(x0s, np.float32).reshape(shape))
        x1 = np.ascontiguousarray(C.to_numpy(x1s, np.float32).reshape(shape))
        B = x0.shape[0]
        b0 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta0s, np.float32).reshape(-1), (B,)))
        b1 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta1s, np.float32).reshape(-1), (B,)))
        tv = None if t is None else np.ascontiguousarray(C.to_numpy(t, np.float32).reshape(B))
        zv = None if z is None else np.ascontiguousarray(C.to_numpy(z, np.float32).reshape(shape))
        kw = self._kw("beta_half", tv, seed, draw, traj_offset, tbins)
        return eng.velocity_loss(x0, x1, b0, b1, z=zv, **kw)


class StandardVelocityLoss(BaseVelocityLoss):
    """l_b = sum [ b+^2 / 2 - (dtIt + gamma' z) b+ + b-^2 / 2 - (dtIt - gamma' z) b- ] over the two antithetic states."""
    KIND = "standard"

    def __init__(self, interpolant: BaseInterpolant, t_distr="uniform") -> None:
        super().__init__(interpolant, t_distr)


class OneSidedVelocityLoss(BaseVelocityLoss):
    """l_b = sum [ b+^2 / 2 - dtIt b+ ]: the noise is x0 itself."""
    KIND = "one_sided"

    def __init__(self, interpolant: BaseInterpolant, t_distr="uniform") -> None:
        super().__init__(interpolant, t_distr)
