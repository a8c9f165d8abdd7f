"""FCNetMultiBeta(d, d, H, L) for toy systems in 1 <= d <= 16 dimensions (Müller-Brown, multi-well potentials) on top of
libti_hip.so (ti_adw_create_nd).

  FCNetMultiBeta      <- /root/reference/adw/thermo/models/simple.py:11-41 with in_size = out_size = d
  ODEWrapper          <- /root/reference/adw/thermo/models/ode_wrapper.py:30-67  (xs [B, d]; divergence = sum_i d b_i / d x_i * 1e-2)
  StandardIntegrator  <- /root/reference/adw/thermo/integrators.py:33-68         (x0s [B, d] -> path [n_step, B, d], dlogp [n_step, B, 1])

Same classes as thermo.adw (which keeps the reference sampler's 1-D contract); the wrapper and the integrator are shared, only the
model shell accepts d > 1.  The reference's own ODEWrapper.forward builds ts = ones_like(xs) * t, which concatenates into the net
only at d = 1; here the time enters as one value per row, which is what the reference net accepts at any d.
"""
from __future__ import annotations

from . import adw as _adw
from .adw import ODEWrapper, StandardIntegrator  # noqa: F401

MAX_DIM = 16                                  # 1 <= d <= MAX_DIM (ti_adw_create_nd)


class FCNetMultiBeta(_adw.FCNetMultiBeta):
    """thermo.adw.FCNetMultiBeta for in_size = out_size = d, 1 <= d <= 16.  from_torch_module infers d from net.0.weight."""

    @staticmethod
    def _check_sizes(in_size, out_size):
        if in_size != out_size:
            raise ValueError(f"FCNetMultiBeta({in_size}, {out_size}, ...) is not an ODE drift: the HIP path needs in_size == out_size")
        if not 1 <= in_size <= MAX_DIM:
            raise NotImplementedError(f"the HIP path covers in_size = out_size = d with 1 <= d <= {MAX_DIM}, got {in_size}")
