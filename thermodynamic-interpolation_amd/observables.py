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

Bootstrap intervals (ti_obs_bootstrap): ``bootstrap`` and the wrappers ``ess_ti``, ``free_energy_tfep``, ``free_energy_bg`` mirror the
gen_* functions of the reference's mdqm9/analysis/results_00031.py -- a point estimate with a percentile interval over resamples
drawn and reduced on the GPU, after the reference's IQR outlier filter.

Generator EDMD on random Fourier features (ti_obs_rff_gram): ``rff_gram`` contracts the feature Gram matrices of bootstrap resamples
in fp64 on the GPU; ``gedmd_spectrum`` / ``gedmd_generator`` turn them into the implied-timescale eigenvalues of the reference's
adw/analysis/reweight_gedmd.py with their bootstrap interval.  The p x p algebra is host numpy by default; ``solver="device"`` runs it
on the GPU too (ti_obs_gedmd_spectrum: a batched Hermitian Jacobi eigensolver in LDS, ``eigh_batched`` on its own), p <= 64.
``rff_gram_wide`` (ti_obs_rff_gram_wide) is the same contraction up to p = 1024, the molecule study's size (mdqm9/analysis/gedmd.py,
p = 300); ``gedmd_cv`` / ``gedmd_model_selection`` are the reference's cross-validated choice of (sigma, p) (gedmd/rff.py
cv_generator_rff and the two model_selection.py scripts), scored by ``gedmd_vamp_score`` from held-out Gram matrices.

Z-matrix coordinates (ti_obs_zmat, ti_obs_zmat_xyz, ti_obs_hist_cols; zmatrix.py, re-exported here): ``zmatrix`` / ``zmatrix_xyz`` are
the reference's construct_z_matrix_batch / deconstruct_z_matrix_batch with its log-determinant and validity screen,
``zmatrix_marginals`` the weighted marginals of all 3A - 6 internal coordinates in one call, ``iqr_keep`` its IQR keep mask.

TICA (ti_obs_tica_moments, ti_obs_tica_fit, ti_obs_tica_transform): ``tica_fit`` is the reference's
deeptime.decomposition.TICA(lagtime, dim) on the (cos, sin) encoding of torsions (mdqm9/plots/10506_main.ipynb, cell 3) at many lags
in one call over ragged trajectories, ``tica_transform`` the projection, ``tica_marginals`` the weighted histograms of the projected
samples; the estimator is restated in include/ti_hip.h and parity with deeptime's own numbers is not pinned.

Beyond that p x p algebra the only arithmetic in this module is turning a histogram into a free-energy profile, forming phi from
its terms, and the difference of two bootstrap runs in ``free_energy_bg``.
"""
from __future__ import annotations

import collections

import numpy as np

from . import _lib
from .zmatrix import (ZMatrix, ZMarginals, bond_angles, bond_lengths, iqr_keep, torsions, zmatrix, zmatrix_marginals,  # noqa: F401
                      zmatrix_xyz)

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


BootstrapResult = collections.namedtuple("BootstrapResult", "point ci estimates n_kept")
BootstrapResult.__doc__ = """point: the estimate of the (filtered) sample; ci: (lower, upper) percentiles of the resample estimates;
estimates [n_boot] float64 (where logw lives); n_kept: samples the point estimate's filter kept."""


def bootstrap(logw, estimator, k=None, filter=None, n_boot=1000, seed=0, level=0.95, indices=None, first=0, engine=None):
    """Point estimate and percentile interval of `estimator` ('ess', 'tfep' = -ln<exp(logw)>, 'mean' = -<logw>) of logw = -phi [n]
    float32 (numpy or CUDA tensor).  k: the IQR multiple of the reference's filter_iqr, None: no filter.  filter: 'none', 'once' (the
    sample is filtered once and resampled from the survivors: gen_ess_ti), 'resample' (every resample of the whole sample is filtered
    by its own quartiles: gen_free_energy_*); default 'none' without k, else 'once' for 'ess' and 'resample' for the free energies, as
    the reference pairs them.  Resample r is global resample first + r of the stream `seed` (ranks can split one bootstrap);
    indices [n_boot, n_draw] int32 replaces the generator's draws."""
    if estimator not in _lib.BOOT_ESTIMATORS:
        raise ValueError(f"estimator must be one of {sorted(_lib.BOOT_ESTIMATORS)}, got {estimator!r}")
    if filter is None:
        filter = "none" if k is None else "once" if estimator == "ess" else "resample"
    if filter not in _lib.BOOT_FILTERS:
        raise ValueError(f"filter must be one of {sorted(_lib.BOOT_FILTERS)}, got {filter!r}")
    if filter != "none" and (k is None or not np.isfinite(k) or k <= 0):
        raise ValueError(f"filter {filter!r} needs a finite k > 0, got {k!r}")
    if isinstance(n_boot, bool) or int(n_boot) != n_boot or not 0 <= int(n_boot) <= _lib.BOOT_MAX_RESAMPLES:
        raise ValueError(f"n_boot must be an integer in 0..{_lib.BOOT_MAX_RESAMPLES}, got {n_boot!r}")
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must be in (0, 1), got {level!r}")
    if len(logw.shape) != 1 or int(logw.shape[0]) < 1:
        raise ValueError("logw must be 1-D and non-empty")
    eng = engine or _service_engine(_device_of(logw))
    point, lo, hi, kept, est = eng.bootstrap(logw, _lib.BOOT_ESTIMATORS[estimator], _lib.BOOT_FILTERS[filter], 1.0 if k is None else float(k),
                                             float(level), int(n_boot), int(first), int(seed), indices)
    return BootstrapResult(point, (lo, hi), est, kept)


def sample_rff_gaussian(d, p, sigma, seed):
    """Omega [d, p] float64 of a Gaussian kernel of bandwidth sigma: RandomState(seed).randn(d, p) / sigma -- the reference's draw
    (adw/analysis/reweight_gedmd.py), with a seed."""
    if int(d) < 1 or int(p) < 1 or not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"need d >= 1, p >= 1 and a finite sigma > 0, got {(d, p, sigma)}")
    return np.random.RandomState(seed).randn(int(d), int(p)) / float(sigma)


def _check_gram_args(values, omega, n_boot, max_p=_lib.GRAM_MAX_P):
    omega = np.asarray(omega, np.float64)
    if omega.ndim != 2 or not 1 <= omega.shape[0] <= _lib.GRAM_MAX_D or not 1 <= omega.shape[1] <= max_p:
        raise ValueError(f"omega must be [d, p] with 1 <= d <= {_lib.GRAM_MAX_D} and 1 <= p <= {max_p}, got {omega.shape}")
    if not np.isfinite(omega).all():
        raise ValueError("omega must be finite")
    if isinstance(n_boot, bool) or int(n_boot) != n_boot or not 0 <= int(n_boot) <= _lib.BOOT_MAX_RESAMPLES:
        raise ValueError(f"n_boot must be an integer in 0..{_lib.BOOT_MAX_RESAMPLES}, got {n_boot!r}")
    if len(values.shape) not in (1, 2) or int(values.shape[0]) < 1:
        raise ValueError("values must be [n] or [n, d] and non-empty")
    P = -(-omega.shape[1] // 16) * 16
    if int(values.shape[0]) * P > _lib.GRAM_MAX_TABLE:
        raise ValueError(f"n * P = {int(values.shape[0]) * P} exceeds the feature table's cap of 2^27 entries (P = p rounded up to 16)")
    return omega


def rff_gram(values, omega, logw=None, n_boot=0, seed=0, first=0, indices=None, engine=None):
    """G [1 + n_boot, p, p] complex128 (where values lives): the weighted Gram matrices M^H diag(w) M of the random Fourier features
    M = exp(-i values @ omega) -- values [n] or [n, d] float32, omega [d, p] float64 on the host, w = exp(logw - max logw) (None: 1)
    -- over all n samples (row 0) and over n_boot bootstrap resamples, drawn as in ``bootstrap`` (or given by indices
    [n_boot, n_draw] int32), contracted in fp64 on the GPU (ti_obs_rff_gram)."""
    omega = _check_gram_args(values, omega, n_boot)
    eng = engine or _service_engine(_device_of(values, logw))
    return eng.rff_gram(values, omega, logw, int(n_boot), int(first), int(seed), indices)


def rff_gram_wide(values, omega, logw=None, n_boot=0, seed=0, first=0, indices=None, engine=None):
    """``rff_gram`` for p <= 1024 (ti_obs_rff_gram_wide): the same arguments and the same G [1 + n_boot, p, p] complex128 where values
    lives.  Up to p = 128 it is ``rff_gram`` bit for bit; beyond, the columns are contracted panel pair by panel pair, and every
    16 x 16 tile still holds the bits ``rff_gram`` gives for that pair of column tiles of omega."""
    omega = _check_gram_args(values, omega, n_boot, _lib.GRAM_WIDE_MAX_P)
    eng = engine or _service_engine(_device_of(values, logw))
    return eng.rff_gram_wide(values, omega, logw, int(n_boot), int(first), int(seed), indices)


SOLVERS = ("host", "device")


def _check_solver(solver, p):
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if solver == "device" and p > _lib.EIGH_MAX_N:
        raise ValueError(f"solver='device' takes p <= {_lib.EIGH_MAX_N} (the matrices live in LDS), got p = {p}: use solver='host', or the "
                         f"blocked device route gedmd_spectrum_wide / gedmd_generator_wide (p <= {_lib.EIGH_WIDE_MAX_N})")


def _check_spectrum_args(gram, p, a, nev, tol):
    shape = tuple(gram.shape) if hasattr(gram, "shape") else np.shape(gram)
    if shape[-2:] != (p, p):
        raise ValueError(f"gram must be [.., {p}, {p}], got {shape}")
    if isinstance(nev, bool) or int(nev) != nev or not 1 <= int(nev) <= p:
        raise ValueError(f"nev must be an integer in 1..p = {p}, got {nev!r}")
    if not np.isfinite(a) or not np.isfinite(tol) or tol < 0:
        raise ValueError(f"a must be finite and tol finite and >= 0, got {(a, tol)}")


def _device_spectrum(call, gram, omega, a, nev, tol):
    ev, vec, rank = call(gram, omega, a, int(nev), tol)
    host = lambda t: t.detach().cpu().numpy() if hasattr(t, "data_ptr") else t
    return host(ev), host(vec), host(rank).astype(np.int64)


def eigh_batched(a, vectors=True, engine=None):
    """(w [.., n] float64 ascending, v [.., n, n] complex128 -- None without vectors --, sweeps [..] int32) of a stack a [.., n, n] of
    Hermitian matrices, n <= 64, on the GPU (ti_obs_eigh): numpy.linalg.eigh(a, UPLO="U") by parallel cyclic Jacobi, one workgroup
    per matrix, bit for bit the same for a matrix wherever it stands in the stack.  Lives where a lives."""
    return (engine or _service_engine(_device_of(a))).eigh(a, vectors=vectors)


def gedmd_spectrum(gram, omega, a, nev, tol=0.0, solver="host", engine=None):
    """Reversible generator EDMD from Gram matrices (batched over the leading axes of gram [.., p, p]; solver "host": numpy, "device":
    the same algebra on the GPU, p <= 64, a CUDA-tensor gram stays there and only the three results come back): what the
    reference's gedmd/rff.py spectral_analysis_rff_generator(reversible=True) computes through an SVD of M^H, here from G = M^H M.
    eigh(G) in descending order, s = sqrt(max(lambda, 0)), r = max(#{s / s_0 >= tol}, nev), L = U[:, :r] / s[:r],
    R = L^H (-a / 2 (omega^T omega) o G) L, eigh of its Hermitian part; returns (d [.., nev] the last nev eigenvalues in ascending
    order, W [.., p, nev] = L Wi, r [..]).  a is the constant diffusion (a float, 2 / beta in the reference's use).  Tensor-valued
    diffusion, the non-reversible branch and finite-lag Koopman estimation are out of scope."""
    omega = np.asarray(omega, np.float64)
    p = omega.shape[1]
    _check_solver(solver, p)
    _check_spectrum_args(gram, p, a, nev, tol)
    if solver == "device":
        return _device_spectrum((engine or _service_engine(_device_of(gram))).gedmd_spectrum, gram, omega, a, nev, tol)
    G = np.asarray(gram.detach().cpu().numpy() if hasattr(gram, "data_ptr") else gram, np.complex128)
    nev, lead = int(nev), G.shape[:-2]
    G = G.reshape(-1, p, p)
    lam, U = np.linalg.eigh(G)
    lam, U = lam[:, ::-1], U[:, :, ::-1]
    s = np.sqrt(np.maximum(lam, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        rank = np.maximum((s / s[:, :1] >= tol).sum(axis=1), nev)
    ML = (-0.5 * float(a)) * (omega.T @ omega) * G
    d, W = np.zeros((G.shape[0], nev)), np.zeros((G.shape[0], p, nev), np.complex128)
    for r in np.unique(rank):                          # matrices of one rank share the batched calls
        sel = np.flatnonzero(rank == r)
        with np.errstate(divide="ignore"):
            L = U[sel][:, :, :r] / s[sel][:, None, :r]
        Rm = np.conj(np.swapaxes(L, 1, 2)) @ ML[sel] @ L
        di, Wi = np.linalg.eigh(0.5 * (Rm + np.conj(np.swapaxes(Rm, 1, 2))))
        d[sel] = di[:, -nev:]
        W[sel] = L @ Wi[:, :, -nev:]
    return d.reshape(*lead, nev), W.reshape(*lead, p, nev), rank.reshape(lead)


def eigh_batched_wide(a, vectors=True, engine=None):
    """``eigh_batched`` for n <= 1024 (ti_obs_eigh_wide).  Up to n = 64 it is ``eigh_batched`` bit for bit; beyond, a blocked two-sided
    Jacobi method works on 32-wide index blocks from global memory (one LDS Jacobi sweep per visit of a block pair) and sweeps counts
    its outer sweeps.  Bit for bit the same for a matrix wherever it stands in the stack.  Lives where a lives."""
    return (engine or _service_engine(_device_of(a))).eigh_wide(a, vectors=vectors)


def gedmd_spectrum_wide(gram, omega, a, nev, tol=0.0, engine=None):
    """``gedmd_spectrum`` on the GPU for p <= 1024 (ti_obs_gedmd_spectrum_wide): the same definitions, checks and return types; both
    solves by ``eigh_batched_wide``'s method.  p <= 64 gives the bits of ``gedmd_spectrum(solver="device")``.  A CUDA-tensor gram
    stays on the GPU and only the three results come back."""
    omega = np.asarray(omega, np.float64)
    p = omega.shape[1]
    if p > _lib.EIGH_WIDE_MAX_N:
        raise ValueError(f"gedmd_spectrum_wide takes p <= {_lib.EIGH_WIDE_MAX_N}, got p = {p}: use gedmd_spectrum(solver='host')")
    _check_spectrum_args(gram, p, a, nev, tol)
    return _device_spectrum((engine or _service_engine(_device_of(gram))).gedmd_spectrum_wide, gram, omega, a, nev, tol)


GedmdResult = collections.namedtuple("GedmdResult", "eigenvalues ci estimates eigenvectors rank")
GedmdResult.__doc__ = """eigenvalues [nev]: the generator eigenvalues of the whole sample, ascending (the last is ~0; the reference reports
their negatives); ci [2, nev]: percentiles of the resample estimates; estimates [n_boot, nev]; eigenvectors [p, nev] and rank of the
point estimate."""


def gedmd_generator(values, omega, nev, a, tol=0.0, logw=None, n_boot=1000, level=0.95, seed=0, first=0, indices=None, engine=None, solver="host"):
    """The bootstrapped generator spectrum of the reference's adw/analysis/reweight_gedmd.py (bootstrap_eigenvalues over gedmd): the
    Gram matrices on the GPU (``rff_gram``; ``rff_gram_wide`` for 128 < p <= 1024, the molecule study's size), the p x p algebra on the host or, with solver="device", on the GPU as well
    (``gedmd_spectrum``), the interval by numpy's linear percentile rule as in ``bootstrap``.  The reference reweights by weighted resampling and then bootstraps uniformly; here logw
    enters the Gram matrices directly -- the expectation of that step -- and the bootstrap draws uniformly.  The reference's exact
    procedure stays reachable through indices."""
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must be in (0, 1), got {level!r}")
    _check_solver(solver, np.shape(omega)[-1] if np.ndim(omega) else 0)
    gram = rff_gram_wide if np.ndim(omega) == 2 and np.shape(omega)[1] > _lib.GRAM_MAX_P else rff_gram
    G = gram(values, omega, logw=logw, n_boot=n_boot, seed=seed, first=first, indices=indices, engine=engine)
    return _generator_result(*gedmd_spectrum(G, omega, a, nev, tol, solver=solver, engine=engine), level)


def _generator_result(d, W, r, level):
    est = d[1:]
    ci = np.full((2, d.shape[1]), np.nan)
    if est.shape[0] and not np.isnan(est).any():
        ci = np.percentile(est, [50 * (1 - float(level)), 50 * (1 + float(level))], axis=0)
    return GedmdResult(d[0], ci, est, W[0], int(r[0]))


def gedmd_generator_wide(values, omega, nev, a, tol=0.0, logw=None, n_boot=1000, level=0.95, seed=0, first=0, indices=None, engine=None):
    """``gedmd_generator`` with the whole chain on the GPU for p <= 1024: ``rff_gram_wide``, then ``gedmd_spectrum_wide`` on the Gram
    stack where it lies, then the same percentile rule.  Only the spectra, the point estimate's eigenvectors and the ranks come back."""
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must be in (0, 1), got {level!r}")
    G = rff_gram_wide(values, omega, logw=logw, n_boot=n_boot, seed=seed, first=first, indices=indices, engine=engine)
    return _generator_result(*gedmd_spectrum_wide(G, omega, a, nev, tol, engine=engine), level)


def gedmd_vamp_score(gram_test, omega, a, W):
    """The VAMP score of the subspace W [.., p, r] on held-out data, from the held-out Gram matrix gram_test [.., p, p] alone (host
    numpy, batched over the leading axes): the reference's gedmd/rff.py _score_test_data_generator, whose SVD of (M_test W)^H is the
    eigendecomposition of C = W^H G_test W here.  C's Hermitian part is taken; eigh(C) = (lambda, U0); L0 = W U0 / sqrt(lambda);
    R = L0^H (-a / 2 (omega^T omega) o G_test) L0; the score is the sum of the eigenvalues of R's Hermitian part.  NaN where a
    lambda is not positive."""
    omega = np.asarray(omega, np.float64)
    if omega.ndim != 2:
        raise ValueError(f"omega must be [d, p], got {omega.shape}")
    p = omega.shape[1]
    host = lambda t: t.detach().cpu().numpy() if hasattr(t, "data_ptr") else t
    G, W = np.asarray(host(gram_test), np.complex128), np.asarray(host(W), np.complex128)
    if G.shape[-2:] != (p, p):
        raise ValueError(f"gram_test must be [.., {p}, {p}], got {G.shape}")
    if W.ndim < 2 or W.shape[-2] != p or not 1 <= W.shape[-1] <= p or W.shape[:-2] != G.shape[:-2]:
        raise ValueError(f"W must be [.., {p}, r] with 1 <= r <= {p} and the leading axes of gram_test, got {W.shape}")
    if not np.isfinite(a):
        raise ValueError(f"a must be finite, got {a!r}")
    herm = lambda A: 0.5 * (A + np.conj(np.swapaxes(A, -1, -2)))
    WH = np.conj(np.swapaxes(W, -1, -2))
    lam, U0 = np.linalg.eigh(herm(WH @ G @ W))
    bad = ~(lam > 0.0).all(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        L0 = (W @ U0) / np.sqrt(lam)[..., None, :]
    L0 = np.where(bad[..., None, None], 0.0, L0)
    ML = (-0.5 * float(a)) * (omega.T @ omega) * G
    score = np.linalg.eigvalsh(herm(np.conj(np.swapaxes(L0, -1, -2)) @ ML @ L0)).sum(axis=-1)
    return np.where(bad, np.nan, score)


GedmdCvResult = collections.namedtuple("GedmdCvResult", "eigenvalues scores rank")
GedmdCvResult.__doc__ = """eigenvalues [ntest, nev]: the generator eigenvalues of every training set, ascending; scores [ntest]: the VAMP score
of its eigenvectors on the held-out set; rank [ntest]: the rank the cutoff kept."""


def gedmd_cv(values, omega, a, nev, tol=0.0, rtrain=0.75, ntest=20, seed=0, splits=None, logw=None, engine=None):
    """The reference's gedmd/rff.py cv_generator_rff: ntest random splits of the sample into a training share rtrain and a held-out
    rest; the generator spectrum of the training set (``gedmd_spectrum``, host algebra) and the VAMP score of its nev eigenvectors
    on the held-out set (``gedmd_vamp_score``).  Both need the two Gram matrices only: two ``rff_gram_wide`` calls with the splits as
    indices, on the GPU.
    splits [ntest, n] int32 holds one permutation of 0..n-1 per row: the first floor(rtrain n) entries are the training set, the
    rest the held-out set (sklearn's train_test_split sizes for a float train_size).  None: RandomState(seed).permutation(n) per row.
    The score has the sign of the reference FUNCTION (a sum of generator eigenvalues, <= 0, larger is better); the reference's
    model_selection.py scripts store its negative."""
    n = int(values.shape[0])
    if not 0.0 < float(rtrain) < 1.0:
        raise ValueError(f"rtrain must be in (0, 1), got {rtrain!r}")
    ntr = int(np.floor(float(rtrain) * n))
    if ntr < 1 or n - ntr < 1:
        raise ValueError(f"rtrain = {rtrain} of n = {n} samples leaves the training or the held-out set empty")
    if isinstance(nev, bool) or int(nev) != nev or not 1 <= int(nev) <= ntr:
        raise ValueError(f"nev must be an integer in 1..{ntr} (the training size), got {nev!r}")
    if splits is None:
        if isinstance(ntest, bool) or int(ntest) != ntest or int(ntest) < 1:
            raise ValueError(f"ntest must be an integer >= 1, got {ntest!r}")
        rs = np.random.RandomState(seed)
        splits = np.stack([rs.permutation(n) for _ in range(int(ntest))])
    splits = np.asarray(splits.detach().cpu().numpy() if hasattr(splits, "data_ptr") else splits)
    if splits.ndim != 2 or splits.shape[1] != n or splits.shape[0] < 1:
        raise ValueError(f"splits must be [ntest, n = {n}], got {splits.shape}")
    if not (np.sort(splits, axis=1) == np.arange(n)).all():
        raise ValueError("every row of splits must be a permutation of 0..n-1")
    splits = np.ascontiguousarray(splits, np.int32)
    train, test = np.ascontiguousarray(splits[:, :ntr]), np.ascontiguousarray(splits[:, ntr:])
    if hasattr(values, "data_ptr") and values.is_cuda:
        import torch
        train, test = (torch.from_numpy(t).to(values.device) for t in (train, test))
    # each call also forms the row of all n samples (row 0), which is dropped: about 1 / (ntest rtrain) extra Gram work, small beside
    # the host algebra below
    kw = dict(logw=logw, n_boot=splits.shape[0], engine=engine)
    Gtr = rff_gram_wide(values, omega, indices=train, **kw)[1:]
    Gte = rff_gram_wide(values, omega, indices=test, **kw)[1:]
    d, W, r = gedmd_spectrum(Gtr, omega, a, nev, tol, solver="host")
    return GedmdCvResult(d, gedmd_vamp_score(Gte, omega, a, W), r)


def gedmd_model_selection(values, sigmas, ps, a, nev, tol=0.0, seed=0, rtrain=0.75, ntest=20, logw=None, engine=None):
    """The double loop of the reference's adw/analysis/model_selection.py and mdqm9/analysis/model_selection.py: ``gedmd_cv`` at every
    (sigma, p) of the grid, Omega drawn per grid point by ``sample_rff_gaussian``(d, p, sigma, seed) and the splits by `seed`.
    Returns (EV [len(sigmas), len(ps), ntest, nev], VAMP [len(sigmas), len(ps), ntest])."""
    sigmas, ps = list(sigmas), [int(p) for p in ps]
    d = 1 if len(values.shape) == 1 else int(values.shape[1])
    EV, VAMP = np.zeros((len(sigmas), len(ps), int(ntest), int(nev))), np.zeros((len(sigmas), len(ps), int(ntest)))
    for i, sigma in enumerate(sigmas):
        for j, p in enumerate(ps):
            cv = gedmd_cv(values, sample_rff_gaussian(d, p, float(sigma), seed), a, nev, tol, rtrain, ntest, seed, logw=logw, engine=engine)
            EV[i, j], VAMP[i, j] = cv.eigenvalues, cv.scores
    return EV, VAMP


def _neg_phi(*terms):
    """-(sum of the terms) formed in fp64 and rounded to fp32 once; a CUDA tensor if any term is one."""
    if any(hasattr(t, "data_ptr") for t in terms):
        import torch
        dev = next((t.device for t in terms if hasattr(t, "data_ptr") and t.is_cuda), None)
        phi = sum(torch.as_tensor(t, device=dev).to(torch.float64).reshape(-1) for t in terms)
        return (-phi).to(torch.float32).contiguous()
    return (-sum(np.asarray(t, np.float64).reshape(-1) for t in terms)).astype(np.float32)


def _neg(a):
    return -a if hasattr(a, "data_ptr") else -np.asarray(a, np.float64)


def ess_ti(E0, E1, neg_dlogp, k=None, **kw):
    """gen_ess_ti: the ESS of the TI map's weights exp(-phi), phi = E1 - E0 + neg_dlogp, filtered once when k is given."""
    return bootstrap(_neg_phi(E1, _neg(E0), neg_dlogp), "ess", k=k, **kw)


def free_energy_tfep(E0, E1, neg_dlogp, k=None, **kw):
    """gen_free_energy_tfep_md_ti (and, with E_T1 + neg_dlogp_T1 - neg_dlogp_T0 folded into the terms, gen_free_energy_bg_tfep):
    dF = -ln<exp(-phi)>, phi = E1 - E0 + neg_dlogp; with k every resample is filtered on exp(-phi) by its own quartiles."""
    return bootstrap(_neg_phi(E1, _neg(E0), neg_dlogp), "tfep", k=k, **kw)


def free_energy_bg(E_T0, neg_dlogp_T0, E_T1, neg_dlogp_T1, k=None, seed=0, **kw):
    """gen_free_energy_bg: dF = <phi1> - <phi0>, phi_i = E_Ti + neg_dlogp_Ti; the two samples are resampled independently (two calls,
    seeds 2 seed and 2 seed + 1) and the interval is taken over the differences of their estimates."""
    level = float(kw.get("level", 0.95))
    r0 = bootstrap(_neg_phi(E_T0, neg_dlogp_T0), "mean", k=k, seed=2 * int(seed), **kw)
    r1 = bootstrap(_neg_phi(E_T1, neg_dlogp_T1), "mean", k=k, seed=2 * int(seed) + 1, **kw)
    if r0.estimates is None:
        return BootstrapResult(r1.point - r0.point, (float("nan"), float("nan")), None, (r0.n_kept, r1.n_kept))
    diff = r1.estimates - r0.estimates
    host = diff.detach().cpu().numpy() if hasattr(diff, "data_ptr") else diff
    ci = (float("nan"), float("nan")) if np.isnan(host).any() else tuple(np.percentile(host, [50 * (1 - level), 50 * (1 + level)]))
    return BootstrapResult(r1.point - r0.point, ci, diff, (r0.n_kept, r1.n_kept))


def ff_energy(engine, x, to_nm=1.0, T=None, terms=False):
    """E [B] float64 of x [B,A,3] float32 under the force field set on `engine` (PainnEngine.set_forcefield), evaluated on the GPU in
    fp64 at the positions x * to_nm: kJ/mol, or with T [B] kelvin the reduced energy E / (R T) the estimators above take as E0s / E1s.
    terms=True: (E, [B, 4] bond, angle, torsion and pair sums).  Lives where x lives."""
    return engine.ff_energy(x, to_nm=to_nm, T=T, terms=terms)


def ff_forces(engine, x, to_nm=1.0, T=None, energy=False):
    """F [B,A,3] float64 = -dE / d(position in nm) of x [B,A,3] float32 under the force field set on `engine`, evaluated on the GPU in
    fp64 at the positions x * to_nm: kJ / (mol nm), or with T [B] kelvin divided by R T.  energy=True: (F, E [B]) with the energy of the
    same pass.  Lives where x lives."""
    return engine.ff_forces(x, to_nm=to_nm, T=T, energy=energy)


def ti_logw(u0, u1, neg_dlogp, engine=None):
    """logw [B] float32 = -(u1 - u0 + neg_dlogp) from reduced energies u0, u1 [B] float64 (u0 None: 0, the calc_phis_bg form) and
    neg_dlogp [B] float32 (None: 0), formed in fp64 on the GPU and rounded once: what ``importance_weights``, ``weighted_histogram``,
    ``bootstrap`` and ``rff_gram`` take.  Lives where u1 lives."""
    return (engine or _service_engine(_device_of(u1))).ti_logw(u0, u1, neg_dlogp)


def log_prior(z, engine=None):
    """log N(z; 0, I) [B] float64 of the prior samples z [B, ...] float32, each row flattened (the reference's calc_log_mvnormal_pzs):
    -(sum z^2) / 2 - m log(2 pi) / 2 in fp64 on the GPU, a function of the row alone (ti_obs_bg_logw).  Lives where z lives."""
    return (engine or _service_engine(_device_of(z))).bg_logw(z, logpz=True)[1]


def bg_logw(z0, E1, neg_dlogp_bg, neg_dlogp_ti=None, engine=None):
    """logw [B] float32 = -(E1 + log N(z0; 0, I) + neg_dlogp_bg + neg_dlogp_ti): the log of the reference's calc_importance_weights,
    the weight of a Boltzmann generator's sample (neg_dlogp_ti None) or of a latent -> ambient chain's.  z0 [B, ...] float32, E1 [B]
    float64 reduced energies of the generated state (None: 0), the dlogps [B] float32 (None: 0); formed in fp64 on the GPU and
    rounded once: what ``importance_weights``, ``weighted_histogram``, ``bootstrap`` and ``rff_gram`` take.  Lives where z0 lives."""
    return (engine or _service_engine(_device_of(z0))).bg_logw(z0, E1, neg_dlogp_bg, neg_dlogp_ti)


def ess_bg(z0, E1, neg_dlogp_bg, neg_dlogp_ti=None, k=None, **kw):
    """gen_ess_bg: the ESS of the Boltzmann-generator weights, filtered once when k is given.  The interval and the resample
    estimates are ``bootstrap(bg_logw(...), "ess", k=k)``; the point estimate is taken from the unrounded fp64 log-weights
    (ti_obs_bg_ess) over the sample the filter kept, so that it is calc_ESS of the reference's fp64 weights to the summation error --
    the one fp32 rounding of ``bg_logw`` alone would move it by up to 2e-6 relative."""
    eng = kw.get("engine") or _service_engine(_device_of(z0))
    logw, logpz = eng.bg_logw(z0, E1, neg_dlogp_bg, neg_dlogp_ti, logpz=True)
    r = bootstrap(logw, "ess", k=k, **kw)
    keep = None if k is None else iqr_keep(logw, k)
    if keep is not None and hasattr(logw, "data_ptr") and logw.is_cuda:
        import torch
        keep = torch.from_numpy(keep).to(logw.device)
    point, _ = eng.bg_ess(logpz, E1, neg_dlogp_bg, neg_dlogp_ti, keep)
    return BootstrapResult(point, r.ci, r.estimates, r.n_kept)


def free_energy_bg_tfep(E_T0, neg_dlogp_T0, E_T1, neg_dlogp_T1, k=None, **kw):
    """gen_free_energy_bg_tfep: dF = -ln<exp(-phi)>, phi = E_T1 + neg_dlogp_T1 - E_T0 - neg_dlogp_T0 (calc_phis_bg_tfep), the fold
    ``free_energy_tfep`` names; with k every resample is filtered on exp(-phi) by its own quartiles."""
    return bootstrap(_neg_phi(E_T1, neg_dlogp_T1, _neg(E_T0), _neg(neg_dlogp_T0)), "tfep", k=k, **kw)


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


# ---- TICA (ti_obs_tica_moments, ti_obs_tica_fit, ti_obs_tica_transform)
TicaModel = collections.namedtuple("TicaModel", "lags mean eigenvalues components rank timescales encode")
TicaModel.__doc__ = """lags [n_lag] int32; mean [n_lag, d], eigenvalues [n_lag, dim], components [n_lag, d, dim] float64 (where the fitted
values live); rank [n_lag] int32; timescales [n_lag, dim] float64 (numpy): -lag / ln(lambda) in frames for 0 < lambda < 1, else NaN;
encode: "torsion" (d = 2 K, (cos, sin) of every value) or "none" (d = K)."""

_TICA_ENCODINGS = {"torsion": 1, "none": 0}


def _check_tica_args(values, traj_offsets, lags, encode):
    """(traj_offsets int64, lags int32, encode flag) of a TICA request, checked before any device call"""
    if encode not in _TICA_ENCODINGS:
        raise ValueError(f"encode must be one of {sorted(_TICA_ENCODINGS)}, got {encode!r}")
    if len(values.shape) != 2 or int(values.shape[0]) < 1:
        raise ValueError(f"values must be [n, K], got {tuple(values.shape)}")
    n, K = int(values.shape[0]), int(values.shape[1])
    if not 1 <= K <= _lib.TICA_MAX_K:
        raise ValueError(f"values must have 1..{_lib.TICA_MAX_K} columns, got {K}")
    if K * (2 if _TICA_ENCODINGS[encode] else 1) > _lib.EIGH_MAX_N:
        raise ValueError(f"at most {_lib.EIGH_MAX_N} features: K = {K} with encode = {encode!r} gives {2 * K}")
    off = np.asarray(traj_offsets)
    if off.ndim != 1 or off.size < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("traj_offsets must be a 1-D integer array of n_traj + 1 >= 2 entries")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != n or np.any(np.diff(off) <= 0):
        raise ValueError(f"traj_offsets must ascend strictly from 0 to n = {n}")
    lg = np.asarray(lags)
    if lg.ndim != 1 or not 1 <= lg.size <= _lib.TICA_MAX_LAGS or not np.issubdtype(lg.dtype, np.integer):
        raise ValueError(f"lags must be a 1-D integer array of 1..{_lib.TICA_MAX_LAGS} entries")
    if np.any(lg < 1) or np.any(lg > np.iinfo(np.int32).max):
        raise ValueError("every lag must be >= 1")
    lens = np.diff(off)
    for tau in lg:
        pairs = int(np.maximum(lens - int(tau), 0).sum())
        if pairs < 2:
            raise ValueError(f"lag {int(tau)} has {pairs} pairs: at least 2 are needed")
    return off, lg.astype(np.int32), _TICA_ENCODINGS[encode]


def tica_moments(values, traj_offsets, lags, encode="torsion", engine=None):
    """(count [n_lag] int64, sum [n_lag, 2, d], cov [n_lag, 3, d, d] float64): the lagged moments (sx, sy) and (Sxx, Syy, Sxy) of
    values [n, K] float32 -- numpy or a CUDA tensor, read through its strides: torsions z[:, 2:, 2] of a Z-matrix array are fine --
    over the trajectories traj_offsets [n_traj + 1] (frames traj_offsets[t] .. traj_offsets[t + 1] - 1 in time order: the
    replica-major layout generate_md writes) at the lags.  Lives where values lives."""
    off, lg, enc = _check_tica_args(values, traj_offsets, lags, encode)
    return (engine or _service_engine(_device_of(values))).tica_moments(values, off, lg, enc)


def _check_tica_model_args(dim, epsilon, scaling, d):
    if isinstance(dim, bool) or int(dim) != dim or not 1 <= int(dim) <= d:
        raise ValueError(f"dim must be an integer in 1..{d}, got {dim!r}")
    if not (np.isfinite(epsilon) and epsilon >= 0):
        raise ValueError(f"epsilon must be finite and >= 0, got {epsilon!r}")
    if scaling not in _lib.TICA_SCALINGS:
        raise ValueError(f"scaling must be one of {sorted(_lib.TICA_SCALINGS)}, got {scaling!r}")


def tica_timescales(lags, eigenvalues):
    """[n_lag, dim] float64: -lag / ln(lambda) in frames where 0 < lambda < 1, NaN elsewhere"""
    ev = np.asarray(eigenvalues.detach().cpu().numpy() if hasattr(eigenvalues, "data_ptr") else eigenvalues, np.float64)
    out = np.full(ev.shape, np.nan)
    ok = (ev > 0) & (ev < 1)
    tau = np.broadcast_to(np.asarray(lags, np.float64)[:, None], ev.shape)
    out[ok] = -tau[ok] / np.log(ev[ok])
    return out


def tica_fit(values, traj_offsets, lags, dim=2, epsilon=1e-6, scaling="kinetic_map", encode="torsion", engine=None):
    """TICA of values [n, K] at every lag (deeptime's documented reversible estimator, restated in include/ti_hip.h; parity with
    deeptime's own numbers is not pinned): a ``TicaModel`` living where values lives.  The moments never leave the device: host
    values are uploaded once (their K columns only), both stages run on device memory, and only the model comes back -- the bits a
    CUDA tensor of the same values gives."""
    off, lg, enc = _check_tica_args(values, traj_offsets, lags, encode)
    _check_tica_model_args(dim, epsilon, scaling, int(values.shape[1]) * (2 if enc else 1))
    eng = engine or _service_engine(_device_of(values))
    dev = hasattr(values, "data_ptr") and values.is_cuda
    if not dev:
        import torch
        host = values.detach().numpy() if hasattr(values, "data_ptr") else values
        values = torch.from_numpy(np.ascontiguousarray(host, np.float32)).to(f"cuda:{eng.device}")
    count, sm, cov = eng.tica_moments(values, off, lg, enc)
    out = eng.tica_fit(count, sm, cov, int(dim), float(epsilon), _lib.TICA_SCALINGS[scaling])
    mean, ev, comp, rank = out if dev else (a.cpu().numpy() for a in out)
    return TicaModel(lg, mean, ev, comp, rank, tica_timescales(lg, ev), encode)


def tica_transform(model, values, engine=None):
    """[n_lag, B, dim] float32: values [B, K] projected onto the model's components at every lag; lives where values lives."""
    if len(values.shape) != 2 or int(values.shape[0]) < 1:
        raise ValueError(f"values must be [B, K], got {tuple(values.shape)}")
    d = int(model.components.shape[1])
    if int(values.shape[1]) * (2 if _TICA_ENCODINGS[model.encode] else 1) != d:
        raise ValueError(f"the model has {d} features (encode = {model.encode!r}) but values has {int(values.shape[1])} columns")
    dev = hasattr(values, "data_ptr") and values.is_cuda
    mean, comp = model.mean, model.components
    if dev != (hasattr(comp, "data_ptr") and comp.is_cuda):
        if dev:
            import torch
            mean, comp = (torch.as_tensor(np.asarray(a), device=values.device) for a in (mean, comp))
        else:
            mean, comp = mean.detach().cpu().numpy(), comp.detach().cpu().numpy()
    return (engine or _service_engine(_device_of(values))).tica_transform(values, mean, comp, _TICA_ENCODINGS[model.encode])


TicaMarginals = collections.namedtuple("TicaMarginals", "hist tails edges")
TicaMarginals.__doc__ = """hist [n_lag, dim, bins], tails [n_lag, dim, 3] (below, at or above, non-finite) float64; edges [bins + 1]"""


def tica_marginals(model, values, logw=None, keep=None, bins=80, range=(-2.5, 2.5), engine=None):
    """The weighted marginal histograms of the projections of values onto every component at every lag (the panels of the
    reference's mdqm9/plots/10506_main.ipynb, cell 3): ti_obs_hist_cols, one call per lag over that lag's dim columns.  logw and keep
    as in ``zmatrix_marginals``."""
    bins, lo, hi = check_bins(bins, range)
    y = tica_transform(model, values, engine=engine)
    eng = engine or _service_engine(_device_of(values))
    L, dim = int(y.shape[0]), int(y.shape[2])
    hist, tails = np.empty((L, dim, bins)), np.empty((L, dim, 3))
    for l in np.arange(L):
        hist[l], tails[l] = eng.hist_cols(y[int(l)], logw, keep, bins, np.full(dim, lo), np.full(dim, hi))
    return TicaMarginals(hist, tails, np.linspace(lo, hi, bins + 1))
