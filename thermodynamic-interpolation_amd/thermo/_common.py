"""Shared host-side helpers of the thermo/ mirror: tensor <-> numpy plumbing and solver-name handling."""
from __future__ import annotations

import numpy as np

# Solver names: torchdiffeq's 'dopri5' (the reference default), 'euler', 'midpoint', 'rk4' restate torchdiffeq
# 0.2.5 (ti_env.yml:14; third-party, absent from the reference checkout -- parity unpinned against the library itself);
# 'heun' and 'em' are build-defined (include/ti_hip.h).
SUPPORTED = ("dopri5", "euler", "midpoint", "rk4", "heun", "em")
NOT_BUILT = ("dopri8", "bosh3", "fehlberg2", "adaptive_heun", "heun2", "heun3", "explicit_adams", "implicit_adams", "fixed_adams",
             "scipy_solver")


def check_method(method: str) -> str:
    if method in SUPPORTED:
        return method
    if method in NOT_BUILT:
        raise NotImplementedError(
            f"method={method!r} is a torchdiffeq solver that is not built here (torchdiffeq is third-party and absent from the "
            f"reference checkout); available: {SUPPORTED}.")
    raise ValueError(f"unknown method {method!r}; expected one of {SUPPORTED}")


STEP_CONTROLS = ("batch", "trajectory")


def check_step_control(step_control: str, method: str) -> str:
    """'batch' (one step size per call, the reference's behaviour) or 'trajectory' (dopri5 only: per-trajectory step control)."""
    if step_control not in STEP_CONTROLS:
        raise ValueError(f"unknown step_control {step_control!r}; expected one of {STEP_CONTROLS}")
    if step_control == "trajectory" and method != "dopri5":
        raise ValueError(f"step_control='trajectory' needs method='dopri5' (got {method!r}): the fixed-grid schemes take no step decisions")
    return step_control


DIVERGENCES = ("exact", "hutchinson")


def check_divergence(divergence: str, n_probes, return_dlogp: bool):
    """'exact' (3A forward-mode passes per molecule, the default) or 'hutchinson' (n_probes Rademacher probes per molecule, fixed for
    the call: unbiased but noisy; include/ti_hip.h ti_painn_drift_div_est).  -> (divergence, n_probes)."""
    if divergence not in DIVERGENCES:
        raise ValueError(f"unknown divergence {divergence!r}; expected one of {DIVERGENCES}")
    if isinstance(n_probes, bool) or not isinstance(n_probes, (int, np.integer)) or n_probes < 1:
        raise ValueError(f"n_probes must be an int >= 1, got {n_probes!r}")
    if divergence == "hutchinson" and not return_dlogp:
        raise ValueError("divergence='hutchinson' estimates dlogp: it needs return_dlogp=True")
    return divergence, int(n_probes)


def is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "detach")


def is_cuda(x) -> bool:
    return is_torch(x) and bool(x.is_cuda)


def as_f32(x, shape):
    """`x` as a float32, C-contiguous [shape] buffer WHERE IT LIVES: a CUDA tensor stays on the GPU (the engine then uses it
    in place through data_ptr(), no host copy), anything else becomes a numpy array."""
    if is_cuda(x):
        import torch
        return x.detach().to(torch.float32).reshape(shape).contiguous()
    return np.ascontiguousarray(to_numpy(x, np.float32).reshape(shape))


def to_numpy(x, dtype=None) -> np.ndarray:
    if is_torch(x):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    return a if dtype is None else a.astype(dtype, copy=False)


def like(result: np.ndarray, template):
    """Return `result` in the container type of `template` (torch tensor on the template's device, or numpy)."""
    if is_torch(result):                          # device-resident path: already a tensor where the inputs live
        return result
    if is_torch(template):
        import torch
        return torch.from_numpy(np.ascontiguousarray(result)).to(template.device)
    return result

