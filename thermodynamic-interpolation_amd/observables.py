"""Observables on the GPU (include/ti_hip.h ti_obs_*): per-molecule collective variables, importance weights, deterministic
weighted histograms, the adw free-energy profile, and the per-row observer of the integrator mirrors.

A descriptor is a tuple whose first entry names the kind:
    ("rmsd",)                 minimal RMSD over proper rotations to `ref` [A,3] (atoms with select != 0; mirror images do not give 0)
    ("dist", i, j)            |x_j - x_i|
    ("angle", i, j, k)        angle at j, radians in [0, pi]
    ("torsion", i, j, k, l)   radians in (-pi, pi]
    ("coord", c)              adw engines only: component c of a particle
with the conventions of the reference's mdqm9/analysis/utils/mol_geometry.py (compute_distance / compute_angle / compute_torsion).
Indices are local to a molecule; in a mixed-species batch a descriptor that names an atom a molecule does not have gives NaN there.

No arithmetic happens in this module apart from turning a histogram into a free-energy profile.
"""
from __future__ import annotations

import numpy as np

from . import _lib

_ARITY = {"rmsd": 0, "dist": 2, "angle": 3, "torsion": 4, "coord": 1}
_NAMES = {v: k for k, v in _lib.OBS_KINDS.items()}


def encode_descriptors(descriptors) -> np.ndarray:
    """[K,5] int32 (kind, i, j, k, l) of a list of descriptor tuples (or of an already encoded array); checks kinds and arities.
    Index ranges are the library's to check: they depend on the engine."""
    if isinstance(descriptors, np.ndarray) and descriptors.ndim == 2 and descriptors.shape[1] == 5:
        descriptors = [(_NAMES.get(int(r[0]), int(r[0])), *map(int, r[1:1 + _ARITY.get(_NAMES.get(int(r[0])), 0)])) for r in descriptors]
    descriptors = list(descriptors)
    if not descriptors:
        raise ValueError("at least one descriptor is needed")
    out = np.zeros((len(descriptors), 5), np.int32)
    for k, d in enumerate(descriptors):
        d = (d,) if isinstance(d, str) else tuple(d)
        kind = d[0].lower() if isinstance(d[0], str) else _NAMES.get(int(d[0]))
        if kind not in _ARITY:
            raise ValueError(f"descriptor {k}: unknown kind {d[0]!r}; expected one of {sorted(_ARITY)}")
        if len(d) - 1 != _ARITY[kind]:
            raise ValueError(f"descriptor {k}: {kind} takes {_ARITY[kind]} indices, got {len(d) - 1}")
        idx = [int(i) for i in d[1:]]
        if any(i < 0 for i in idx):
            raise ValueError(f"descriptor {k}: negative index")
        out[k, 0] = _lib.OBS_KINDS[kind]
        out[k, 1:1 + len(idx)] = idx
    return out


def check_bins(bins, range):
    """(bins, lo, hi) of a histogram request: 1 <= bins <= 256 equal bins on [lo, hi), lo < hi finite."""
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= 256:
        raise ValueError(f"bins must be an integer in 1..256, got {bins!r}")
    lo, hi = (float(v) for v in range)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"range must be finite with lo < hi, got {(lo, hi)}")
    return int(bins), lo, hi


def check_observe(observe):
    """The integrators' ``observe=dict(descriptors=..., ref=None, select=None, every=1)`` -> the same dict, completed and checked."""
    if observe is None:
        return None
    if not isinstance(observe, dict) or "descriptors" not in observe:
        raise ValueError("observe must be a dict with the key 'descriptors' (and optionally 'ref', 'select', 'every')")
    extra = set(observe) - {"descriptors", "ref", "select", "every"}
    if extra:
        raise ValueError(f"observe: unknown keys {sorted(extra)}")
    every = observe.get("every", 1)
    if isinstance(every, bool) or int(every) != every or int(every) < 0:
        raise ValueError(f"observe['every'] must be an integer >= 0, got {every!r}")
    return dict(descriptors=encode_descriptors(observe["descriptors"]), ref=observe.get("ref"), select=observe.get("select"), every=int(every))


_service = {}


def _service_engine(device=0):
    """Weights and histograms need a handle (a stream and a device) but no model: the smallest adw engine, one per device."""
    if device not in _service:
        from . import engine, synthetic, weights as W
        flat = W.flatten_state_dict(synthetic.adw_state_dict(32, 2), W.adw_param_spec(32, 2), dtype=np.float64)
        _service[device] = engine.AdwEngine(32, 2, flat, device=device)
    return _service[device]


def _device_of(*bufs):
    for b in bufs:
        if b is not None and hasattr(b, "data_ptr") and b.is_cuda:
            return int(b.device.index or 0)
    return 0


def collective_variables(engine, x, descriptors, ref=None, select=None):
    """cv [B, K] float32 of x [B,A,3] (PainnEngine) or [B] / [B,d] (AdwEngine); lives where x lives."""
    return engine.collective_variables(x, descriptors, ref=ref, select=select)


def importance_weights(logw, engine=None):
    """(w [B] float32, ess): w = exp(logw) / sum exp(logw), ess = (sum w)^2 / sum w^2 (the reference's calc_ESS)."""
    return (engine or _service_engine(_device_of(logw))).importance_weights(logw)


def weighted_histogram(values, logw, bins, range, engine=None):
    """(hist [bins], tails [3]) float64: the weight per bin of `bins` equal bins on [range[0], range[1]) -- a value on an interior
    edge goes to the upper bin -- and the weight below, at or above the range, and of non-finite values.  logw None: weights 1 / B."""
    check_bins(bins, range)
    return (engine or _service_engine(_device_of(values, logw))).weighted_histogram(values, logw, bins, range)


def free_energy_profile(x, logw, bins=80, range=(-2.5, 2.5), engine=None):
    """F [bins] = -ln p_hat, p_hat the weighted histogram of x normalised over the range and divided by the bin width (a density);
    +inf for empty bins."""
    bins, lo, hi = check_bins(bins, range)
    x1 = x.reshape(-1) if len(x.shape) > 1 else x
    hist, _ = weighted_histogram(x1, logw, bins, (lo, hi), engine=engine)
    return profile_from_histogram(hist, lo, hi)


def profile_from_histogram(hist, lo, hi):
    hist = np.asarray(hist, np.float64)
    total = hist.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        p = hist / (total * (hi - lo) / hist.size) if total > 0 else np.zeros_like(hist)
        return np.where(p > 0, -np.log(p), np.inf)


def end_state_summary(cv, dlogp, bins=32, engine=None):
    """What the drivers write: for every CV column of the end state cv [B,K] its histogram (weighted by exp(-dlogp) when dlogp is
    given) on the column's finite range, the bin edges, and the effective sample size (B without weights)."""
    B, K = int(cv.shape[0]), int(cv.shape[1])
    logw, ess = None, float(B)
    if dlogp is not None:
        logw = -dlogp
        _, ess = importance_weights(logw, engine=engine)
    host = cv.detach().cpu().numpy() if hasattr(cv, "data_ptr") else np.asarray(cv)
    hists, edges = np.zeros((K, bins)), np.zeros((K, bins + 1))
    for k in np.arange(K):
        col = host[:, k][np.isfinite(host[:, k])]
        lo, hi = (float(col.min()), float(col.max())) if col.size else (0.0, 1.0)
        hi = np.nextafter(np.float32(hi), np.float32(np.inf)).astype(np.float64) if hi > lo else lo + 1.0      # the largest value is binned
        hists[k], _ = weighted_histogram(cv[:, int(k)], logw, bins, (lo, float(hi)), engine=engine)
        edges[k] = lo + (float(hi) - lo) * np.arange(bins + 1) / bins
    return hists, edges, ess
