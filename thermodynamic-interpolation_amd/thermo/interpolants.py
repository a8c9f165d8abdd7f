"""Host-side statement of the interpolants the velocity-loss kernels evaluate (include/ti_hip.h ti_painn_vloss), under the reference's
class names and constructor signatures: LinearInterpolant(a=1, gamma='brownian') and OneSidedLinearInterpolant().

An instance is a record of what the library needs -- `kind` ('standard' | 'one_sided'), `gamma_name`, `a_param` -- which
thermo.losses hands to the engine, plus the four functions of the header's formulas on numpy arrays in float64: gamma(t),
gamma_dot(t), It(t, x0, x1), dtIt(t, x0, x1).  The library holds `a` and sig_sum's 2.2 as the float32 values the reference's tensors
hold, so `a_param` is float32(a) and these functions use it.
"""
from __future__ import annotations

import numpy as np

GAMMAS = ("brownian", "sin2", "sig_sum")
SIG_SCALE = float(np.float32(2.2))


def _logistic(u):
    return 1.0 / (1.0 + np.exp(-u))


def gamma_of(name: str, a: float, t):
    """gamma(t) of include/ti_hip.h TI_GAMMA_*"""
    t = np.asarray(t, np.float64)
    if name == "brownian":
        return np.sqrt(a * t * (1.0 - t))
    if name == "sin2":
        return np.sin(np.pi * t) ** 2
    up, um = a * (t - 0.5) + 1.0, a * (t - 0.5) - 1.0
    return SIG_SCALE * (_logistic(up) - _logistic(um) - _logistic(1.0 - a / 2) + _logistic(-1.0 - a / 2))


def gamma_dot_of(name: str, a: float, t):
    """d gamma / d t"""
    t = np.asarray(t, np.float64)
    if name == "brownian":
        return a * (1.0 - 2.0 * t) / (2.0 * np.sqrt(a * t * (1.0 - t)))
    if name == "sin2":
        return 2.0 * np.pi * np.sin(np.pi * t) * np.cos(np.pi * t)
    sp, sm = _logistic(a * (t - 0.5) + 1.0), _logistic(a * (t - 0.5) - 1.0)
    return SIG_SCALE * a * ((1.0 - sp) * sp - (1.0 - sm) * sm)


class BaseInterpolant:
    kind = None
    gamma_name, a_param = "brownian", 1.0

    @staticmethod
    def It(t, x0, x1):
        """(1 - t) x0 + t x1"""
        t = np.asarray(t, np.float64)
        return (1.0 - t) * np.asarray(x0, np.float64) + t * np.asarray(x1, np.float64)

    @staticmethod
    def dtIt(t, x0, x1):
        """x1 - x0"""
        return np.asarray(x1, np.float64) - np.asarray(x0, np.float64)


class LinearInterpolant(BaseInterpolant):
    """xt+- = (1 - t) x0 + t x1 +- gamma(t) z"""
    kind = "standard"

    def __init__(self, a: float = 1, gamma: str = "brownian") -> None:
        if gamma not in GAMMAS:
            raise NotImplementedError(f"gamma must be one of {GAMMAS}, got {gamma!r}")
        self.gamma_name, self.a_param = gamma, float(np.float32(a))

    def gamma(self, t):
        return gamma_of(self.gamma_name, self.a_param, t)

    def gamma_dot(self, t):
        return gamma_dot_of(self.gamma_name, self.a_param, t)


class OneSidedLinearInterpolant(BaseInterpolant):
    """xt = t x1 + (1 - t) x0, x0 being the noise itself: no gamma"""
    kind = "one_sided"

    def __init__(self) -> None:
        pass

    @staticmethod
    def gamma(t):
        return np.zeros_like(np.asarray(t, np.float64))

    gamma_dot = gamma
