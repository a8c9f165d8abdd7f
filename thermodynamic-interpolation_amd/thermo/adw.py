"""Drop-in mirror of the reference adw sampling API on top of libti_hip.so.

  FCNetMultiBeta      <- /root/reference/adw/thermo/models/simple.py:5-41
  ODEWrapper          <- /root/reference/adw/thermo/models/ode_wrapper.py:11-68   (drift and exact divergence)
  StandardIntegrator  <- /root/reference/adw/thermo/integrators.py:11-68

Same class names, constructor arguments and return shapes; tensors in, tensors out (numpy also accepted).  The modules hold
weights only -- all arithmetic runs in the HIP library (fp32 on the device; the reference nets are fp64, adw/train.py:29).
"""
from __future__ import annotations

import numpy as np

from .. import engine as _engine
from .. import observables as _obs
from .. import synthetic as _syn
from .. import weights as _W
from . import _common as C
from . import interpolants, losses  # noqa: F401  (the reference's thermo.interpolants / thermo.losses)


class FCNetMultiBeta:
    """Weights-only shell with the reference constructor signature and state_dict key layout.  This mirror keeps the reference
    sampler's 1-D contract (its ODEWrapper.forward only concatenates at in_size = 1); the d-dimensional model is
    thermo.adw_nd.FCNetMultiBeta, which the ODEWrapper and StandardIntegrator below drive as well."""

    @staticmethod
    def _check_sizes(in_size, out_size):
        if in_size != 1 or out_size != 1:
            raise NotImplementedError("the HIP path covers the reference's 1-D double well (in_size = out_size = 1) here; "
                                      "FCNetMultiBeta(d, d, H, L) for 1 <= d <= 16 is thermo.adw_nd.FCNetMultiBeta")

    def __init__(self, in_size, out_size, hidden_size, num_layers):
        self._check_sizes(in_size, out_size)
        self.in_size, self.out_size, self.hidden_size, self.num_layers = in_size, out_size, hidden_size, num_layers
        self.dim = int(in_size)
        self._spec = _W.adw_param_spec(hidden_size, num_layers, self.dim, self.dim)
        # the reference initialises with torch's default Linear init; weights normally arrive via load_state_dict / torch.load
        self._sd = _syn.make_state_dict(self._spec, seed=0, dtype=np.float64)
        self._engine, self._device = None, 0
        self.precision = "f32"                  # 'f16x2': split-fp16 matrix path; set before first use
        self.training = False

    # -- torch.nn.Module surface used by the sampling driver (adw/sample.py:39, :84-88)
    def state_dict(self):
        return dict(self._sd)

    def load_state_dict(self, state_dict, strict=True):
        flat = _W.flatten_state_dict(state_dict, self._spec, dtype=np.float64, strict=strict)
        self._sd = _W.unflatten(flat, self._spec)
        self._engine = None
        return self

    @classmethod
    def from_torch_module(cls, module):
        """Build from a reference ``FCNetMultiBeta`` instance (what ``torch.load(config.sampling_model)`` returns)."""
        sd = module.state_dict()
        hidden, d = int(sd["net.0.weight"].shape[0]), int(sd["net.0.weight"].shape[1]) - 2
        n_lin = sum(1 for k in sd if k.startswith("net.") and k.endswith(".weight"))
        return cls(d, d, hidden, n_lin - 1).load_state_dict(sd)

    def eval(self):
        self.training = False
        return self

    def double(self):
        return self

    def float(self):
        return self

    def to(self, device=None, *a, **k):
        idx = getattr(device, "index", None)
        if isinstance(device, int):
            idx = device
        elif isinstance(device, str) and ":" in device:
            idx = int(device.split(":")[1])
        if idx is not None and idx != self._device:
            self._device, self._engine = idx, None
        return self

    def parameters(self):
        return iter(self._sd.values())

    def engine(self) -> _engine.AdwEngine:
        if self._engine is None:
            flat = _W.flatten_state_dict(self._sd, self._spec, dtype=np.float64)
            self._engine = _engine.AdwEngine(self.hidden_size, self.num_layers, flat, device=self._device, precision=self.precision,
                                             dim=self.dim)
        return self._engine

    def forward(self, x0s, xts, ts, beta0s, beta1s):
        """net([xts, ts, beta_embed([beta0s, beta1s, ts])]) -> [B, d].  ``x0s`` is unused, as in the reference (simple.py:38-41).
        ``ts``: one value (the sampler passes ones_like(x) * t, ode_wrapper.py:47) or one per row (what training feeds)."""
        if self.dim > 1:
            return self._forward_nd(xts, ts, beta0s, beta1s)
        t = C.to_numpy(ts, np.float32).ravel()
        x = np.ascontiguousarray(C.to_numpy(xts, np.float32).reshape(-1))
        b0 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta0s, np.float32).reshape(-1), x.shape))
        b1 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta1s, np.float32).reshape(-1), x.shape))
        if t.size > 1 and np.ptp(t) != 0.0:
            if t.size != x.size:
                raise ValueError(f"ts must hold one value or one per row ({x.size}), got {t.size}")
            out = self.engine().drift(x, np.ascontiguousarray(t), b0, b1)
        else:
            out = self.engine().drift(x, float(t[0]) if t.size else 0.0, b0, b1)
        return C.like(out.reshape(-1, 1), xts)

    def _forward_nd(self, xts, ts, beta0s, beta1s):
        x = np.ascontiguousarray(C.to_numpy(xts, np.float32).reshape(-1, self.dim))
        B = x.shape[0]
        t = C.to_numpy(ts, np.float32).reshape(B, -1) if np.size(C.to_numpy(ts)) > 1 else C.to_numpy(ts, np.float32).ravel()
        if t.ndim == 2:                          # [B, 1], or ones_like(x) * t: every column of a row must agree
            if np.any(t != t[:, :1]):
                raise ValueError("ts must hold one value or one per row")
            t = t[:, 0]
        b0 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta0s, np.float32).reshape(-1), (B,)))
        b1 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta1s, np.float32).reshape(-1), (B,)))
        if t.size > 1 and np.ptp(t) != 0.0:
            out = self.engine().drift(x, np.ascontiguousarray(t), b0, b1)
        else:
            out = self.engine().drift(x, float(t[0]) if t.size else 0.0, b0, b1)
        return C.like(out, xts)

    __call__ = forward


class ODEWrapper:
    """forward(t, states, x0s, beta0s, beta1s) -> b, or (b, -divergence) with return_dlogp
    (divergence = d b / d x * 1e-2 like ode_wrapper.py:55-67; reverse_ode flips both signs)."""

    def __init__(self, b, return_dlogp=False, reverse_ode=False):
        self.b, self.return_dlogp, self.reverse_ode = b, return_dlogp, reverse_ode

    def forward(self, integration_time, states, x0s, beta0s, beta1s):
        xs = states[0] if isinstance(states, (tuple, list)) else states
        t = float(integration_time)
        if self.b.dim > 1:
            return self._forward_nd(xs, t, beta0s, beta1s)
        if not self.return_dlogp:
            ts = np.full(C.to_numpy(xs).shape, t, np.float32)
            return self.b.forward(x0s, xs, ts, beta0s, beta1s)
        x = np.ascontiguousarray(C.to_numpy(xs, np.float32).reshape(-1))
        b0 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta0s, np.float32).reshape(-1), x.shape))
        b1 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta1s, np.float32).reshape(-1), x.shape))
        b, div = self.b.engine().drift(x, t, b0, b1, return_div=True)
        b, div = C.like(b.reshape(-1, 1), xs), C.like(div * np.float32(1e-2), xs)
        return (b, -div) if not self.reverse_ode else (-b, div)

    def _forward_nd(self, xs, t, beta0s, beta1s):
        d = self.b.dim
        if len(xs.shape) != 2 or xs.shape[1] != d:
            raise ValueError(f"xs must be [batch, {d}]")
        B = int(xs.shape[0])
        if C.is_cuda(xs):                                    # stay in HBM, as StandardIntegrator.rollout does
            import torch
            x = xs.detach().to(torch.float32).contiguous()
            b0 = torch.as_tensor(beta0s, device=x.device).to(torch.float32).reshape(-1).expand(B).contiguous()
            b1 = torch.as_tensor(beta1s, device=x.device).to(torch.float32).reshape(-1).expand(B).contiguous()
        else:
            x = np.ascontiguousarray(C.to_numpy(xs, np.float32))
            b0 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta0s, np.float32).reshape(-1), (B,)))
            b1 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta1s, np.float32).reshape(-1), (B,)))
        if not self.return_dlogp:
            return C.like(self.b.engine().drift(x, t, b0, b1), xs)
        b, div = self.b.engine().drift(x, t, b0, b1, return_div=True)
        b, div = C.like(b, xs), C.like((div * np.float32(1e-2)).reshape(B, 1), xs)
        return (b, -div) if not self.reverse_ode else (-b, div)

    __call__ = forward


class StandardIntegrator:
    """rollout(x0s [B, d], beta0s, beta1s) -> (x [n_saved, B, d], dlogp)   -- reference: (x [n_step, B, d], dlogp * 1e2).

    ``method``: 'dopri5' (adaptive, rtol / atol; the grid selects the output times) or 'euler' | 'midpoint' | 'rk4' | 'heun' | 'em'
    on the grid torch.linspace(start, end, n_step) (n_step - 1 steps).  Extra keyword
    arguments are build-defined: ``eps``/``seed`` (EM noise), ``save_every`` (1 keeps every grid point like the reference;
    0 keeps the end state only).  With return_dlogp=True the second ODE state d(dlogp)/dt = -div * 1e-2 is integrated with the
    same scheme and returned * 1e2 as [n_saved, B, 1], like the reference (integrators.py:38-68).  With return_dlogp=False the
    reference evaluates ``None * 1e2`` and raises (integrators.py:42,68); here dlogp is returned as None instead.
    ``step_control`` (keyword-only): 'batch' (default, one step size per call like the reference's odeint) or 'trajectory'
    (method='dopri5' only: every particle gets the steps the reference takes for it at batch size 1; the per-particle
    (accepted, rejected) counts of the last rollout are then in ``n_steps_per_particle``).
    ``observe`` (keyword-only): dict(descriptors=[("coord", c), ...], every=1) -- the named components of every particle at the grid
    points i % every == 0 and at the last one, whatever save_every is; after rollout they are in ``self.cv`` [rows, B, K] (a CUDA
    tensor when x0s is one).
    ``fused`` (keyword-only, default False): run the whole step loop in one kernel launch (AdwEngine.rollout(fused=True): 1-D model,
    'euler' | 'heun' | 'em', no ``observe``; anything else raises the library's TI_E_UNSUPPORTED) -- the same result bit for bit.
    """

    def __init__(self, b, method: str = "dopri5", n_step: int = 100, atol: float = 1e-4, rtol: float = 1e-4, start: float = 0.0,
                 end: float = 1.0, return_dlogp=False, *, eps: float = 0.0, seed: int = 0, save_every: int = 1,
                 step_control: str = "batch", observe=None, fused: bool = False):
        self.method = C.check_method(method)
        self.step_control = C.check_step_control(step_control, self.method)
        self.observe, self.cv = _obs.check_observe(observe), None
        if self.observe is not None and step_control == "trajectory":
            raise ValueError("observe= is not available with step_control='trajectory' (its rows are written per trajectory)")
        self.ode_wrapper = ODEWrapper(b, return_dlogp=return_dlogp)
        self.start, self.end, self.rtol, self.atol = start, end, rtol, atol
        self.n_step, self.return_dlogp = n_step, return_dlogp
        self.eps, self.seed, self.save_every = eps, seed, save_every
        self.fused = bool(fused)

    def rollout(self, x0s, beta0s, beta1s, traj_offset: int = 0):
        d = self.ode_wrapper.b.dim
        if len(x0s.shape) != 2 or x0s.shape[1] != d:
            raise ValueError(f"x0s must be [batch, {d}]")
        B = int(x0s.shape[0])
        if C.is_cuda(x0s):                                   # stay in HBM: data_ptr() in, CUDA tensors out
            import torch
            x0 = x0s.detach().to(torch.float32).reshape((B,) if d == 1 else (B, d)).contiguous()
            b0 = torch.as_tensor(beta0s, device=x0.device).to(torch.float32).reshape(-1).expand(B).contiguous()
            b1 = torch.as_tensor(beta1s, device=x0.device).to(torch.float32).reshape(-1).expand(B).contiguous()
        else:
            x0 = np.ascontiguousarray(C.to_numpy(x0s, np.float32)[:, 0] if d == 1 else C.to_numpy(x0s, np.float32))
            b0 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta0s, np.float32).reshape(-1), (B,)))
            b1 = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta1s, np.float32).reshape(-1), (B,)))
        grid = _engine.time_grid(self.start, self.end, self.n_step)
        eng = self.ode_wrapper.b.engine()
        if self.observe is not None:
            o = self.observe
            rows = int(_engine._lib.lib().ti_rollout_rows(int(self.n_step), o["every"]))
            self.cv = _engine._alloc_like(x0 if C.is_cuda(x0) else None, (rows, B, int(o["descriptors"].shape[0])))
            eng.set_observer(o["descriptors"], None, None, o["every"], self.cv)
        try:
            res = eng.rollout(x0, b0, b1, grid, scheme=self.method,
                              save_every=self.save_every, eps=self.eps, seed=self.seed, traj_offset=traj_offset,
                              return_dlogp=bool(self.return_dlogp), rtol=self.rtol, atol=self.atol,
                              step_control=self.step_control, fused=self.fused)
        finally:
            if self.observe is not None:
                eng.set_observer(None)
        self.n_fevals = res[-1]
        self.n_steps_per_particle = self.ode_wrapper.b.engine().step_counts(B) if self.step_control == "trajectory" else None
        dlogp = C.like(res[1][:, :, None], x0s) if self.return_dlogp else None
        return C.like(res[0][:, :, None] if d == 1 else res[0], x0s), dlogp


def minibatch_indices(n, batch_size, n_steps, rng):
    """[n_steps, batch_size] int64: rows of a set of n, epoch after epoch a fresh permutation cut into its full batches (drop_last),
    as a shuffling DataLoader hands them out"""
    per = n // batch_size
    if per < 1:
        raise ValueError(f"a set of {n} rows has no full batch of {batch_size}")
    out = []
    while len(out) < n_steps:
        out.extend(rng.permutation(n)[:per * batch_size].reshape(per, batch_size))
    return np.ascontiguousarray(np.stack(out[:n_steps]), np.int64)


class Trainer:
    """The optimiser side of adw/train.py:40-74 on the device (engine.AdwTrainer): loss_fn(b, ...) differentiated, clip_grad_norm_ at
    max_grad_norm, torch.optim.Adam(lr, betas, eps, weight_decay), the NaN skip.  ``b`` is a thermo.adw / thermo.adw_nd
    FCNetMultiBeta whose weights are the starting point; ``loss_fn`` a thermo.losses loss, which gives the kind, gamma, a and
    t_distr.  The fp64 master weights live on the device; ``sync()`` writes them back into ``b``."""

    def __init__(self, b, loss_fn, lr, weight_decay=0.0, max_grad_norm=1.0, betas=(0.9, 0.999), eps=1e-8):
        ip = loss_fn.interpolant
        self.b, self.loss_fn = b, loss_fn
        self._kw = dict(kind=loss_fn.KIND, gamma=ip.gamma_name, a=ip.a_param, t_distr="uniform" if loss_fn.t_distr == "uniform" else "beta_half")
        flat = _W.flatten_state_dict(b._sd, b._spec, dtype=np.float64)
        self.lr = float(lr)
        self.engine = _engine.AdwTrainer(b.hidden_size, b.num_layers, flat, dim=b.dim, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                         max_grad_norm=max_grad_norm, device=b._device)

    def _rows(self, x, beta):
        d = self.b.dim
        x = np.ascontiguousarray(C.to_numpy(x, np.float32).reshape((-1,) if d == 1 else (-1, d)))
        beta = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta, np.float32).reshape(-1), (x.shape[0],)))
        return x, beta

    def _draws(self, t, z, B):
        d = self.b.dim
        tv = None if t is None else np.ascontiguousarray(C.to_numpy(t, np.float32).reshape(B))
        zv = None if z is None else np.ascontiguousarray(C.to_numpy(z, np.float32).reshape((B,) if d == 1 else (B, d)))
        return tv, zv

    def step(self, x0s, x1s, beta0s, beta1s, *, t=None, z=None, seed=0, draw=0, traj_offset=0) -> float:
        """One optimiser step on the batch -> its mean loss (NaN where the step was skipped)"""
        (x0, b0), (x1, b1) = self._rows(x0s, beta0s), self._rows(x1s, beta1s)
        tv, zv = self._draws(t, z, x0.shape[0])
        return self.engine.step(x0, x1, b0, b1, t=tv, z=zv, seed=seed, draw=draw, traj_offset=traj_offset, **self._kw)[0]

    def loss(self, x0s, x1s, beta0s, beta1s, *, t=None, z=None, seed=0, draw=0, traj_offset=0) -> float:
        """The mean loss of the batch at the current weights by the trainer's own forward pass; nothing is updated"""
        (x0, b0), (x1, b1) = self._rows(x0s, beta0s), self._rows(x1s, beta1s)
        tv, zv = self._draws(t, z, x0.shape[0])
        return self.engine.grad(x0, x1, b0, b1, t=tv, z=zv, seed=seed, draw=draw, traj_offset=traj_offset, **self._kw)["mean"]

    def fit(self, x0_all, x1_all, beta0_all, beta1_all, batch_size, n_steps, seed, *, draw=0, noise_seed=None):
        """n_steps optimiser steps in one device loop: minibatches from permutations drawn on the host with `seed`
        (minibatch_indices, independently for the two sets), step k with the (t, z) of draw + k under noise_seed (default: seed).
        -> (mean loss of every step [n_steps], NaN where skipped; the number of skipped steps)"""
        (x0, b0), (x1, b1) = self._rows(x0_all, beta0_all), self._rows(x1_all, beta1_all)
        rng = np.random.default_rng(seed)
        i0 = minibatch_indices(x0.shape[0], batch_size, n_steps, rng)
        i1 = minibatch_indices(x1.shape[0], batch_size, n_steps, rng)
        return self.engine.steps(x0, x1, b0, b1, i0, i1, seed=seed if noise_seed is None else noise_seed, draw=draw, **self._kw)

    def set_lr(self, lr):
        self.engine.set_lr(lr)
        self.lr = float(lr)

    def sync(self):
        """Write the master weights back into ``b`` (load_state_dict: its drift engine is rebuilt on next use) -> b"""
        return self.b.load_state_dict(_W.unflatten(self.engine.weights(), self.b._spec))

    def state_dict(self):
        """The optimiser state for resuming: master weights, moments, counters, learning rate"""
        return dict(self.engine.state(), lr=self.lr)

    def load_state_dict(self, state):
        self.engine.load_state(w=state["w"], m=state["m"], v=state["v"], n_applied=int(state["n_applied"]))
        self.set_lr(float(state["lr"]))
        return self
