"""Sampling drivers with the reference's loop structure and output files.

  sample_ambient <- /root/reference/mdqm9/sample_ambient.py:18-119   samples_/dlogps_/latent_noises_/latent_dlogps_{name}.npy
  sample_latent  <- /root/reference/mdqm9/sample_latent.py:19-96     samples_/dlogps_{name}_forward.npy (dlogps with return_dlogp)
  sample_adw     <- /root/reference/adw/sample.py:14-81              initial_samples/samples/dlogps _epoch_{k}.npy under beta_{b0}_to_{b1}/
  load_config    <- /root/reference/mdqm9/thermo/utils.py:31-47      JSON file -> argparse.Namespace (keys become --options)

Differences, on purpose: `method` comes from ``config.method`` (default 'dopri5' like the reference's hard-coded solver; any
name of thermo._common.SUPPORTED works); files are written once per call instead of re-saving the growing concatenation after every batch
(O(n_batches^2) I/O in the reference); datasets are the numpy ones of ``data.py``.  ``config.step_control`` (optional, default
'batch'): 'trajectory' gives every molecule / particle its own dopri5 step sizes, so its sample and dlogp equal the reference's at
batch size 1 whatever ``batch_size`` is.  ``config.divergence`` / ``n_probes`` / ``probe_seed`` (optional, default 'exact' / 1 / 0):
'hutchinson' estimates dlogp with n_probes Rademacher probes per molecule (MoleculeIntegratorBase); the molecules of successive
batches then get consecutive trajectory ids, so no two molecules of a run share probes.  ``config.observables`` (optional): a dict
``{"descriptors": [["rmsd"], ["torsion", 0, 1, 2, 3], ...], "ref": [[x, y, z], ...], "select": [...], "every": k, "bins": n}``
(observables.py; adw: ``[["coord", 0]]``) writes ``observables_*.npz`` next to the samples file: ``cv`` [rows, B, K], the collective
variables at the grid points i % every == 0 and at the last one, computed on the GPU during the rollout; ``hist`` [K, bins] and
``edges`` [K, bins + 1], the histogram of every CV at the end state, weighted by exp(-dlogp) when ``return_dlogp`` is set; ``ess``.
An integer ``"bootstrap": n`` in that dict adds ``ess_ci`` [2], the 95 % interval of the ESS from n bootstrap resamples drawn on the
GPU (observables.bootstrap, seed 0), and ``ess_boot`` [n], their estimates.  sample_adw only: ``"gedmd": {"p": 50, "sigma": 0.6,
"nev": 4, "tol": 1e-4, "n_boot": 1000, "seed": 0, "potential": [a, b], "solver": "host"}`` (every entry optional; solver "device"
runs the p x p algebra on the GPU too, p <= 64) adds ``gedmd_eigenvalues`` [nev],
``gedmd_ci`` [2, nev] and ``gedmd_rank``: the generator spectrum of the reweighted end state with its bootstrap interval
(observables.gedmd_generator; U = a (x^2 - 1)^2 + b x).  sample_ambient / sample_latent: ``"kinetics": {"columns": [...], "p": 300,
"sigma": 5.0, "nev": 4, "tol": 1e-4, "n_boot": 1000, "seed": 0, "temperature": T}`` (columns and temperature required) adds
``kinetics_eigenvalues`` [nev], ``kinetics_ci`` [2, nev] and ``kinetics_rank``: the unweighted generator spectrum of the selected CV
columns (the torsions; at most 16) of the end-state row, a = k_B T with k_B = 0.008314462618, as the reference's
mdqm9/analysis/gedmd.py computes it; the key is checked before the rollout and refused by sample_adw.  sample_ambient with ``return_dlogp`` only: ``"energy": {"forcefield":
<path of an OpenMM system XML, forcefield.ForceField.from_openmm_xml>, "scale": <SCALING_FACTOR of the species>}`` evaluates the
reduced force-field energies on the GPU (observables.ff_energy at to_nm = 1 / scale, eval_energy.py:77-78): E0 of every x0 at its T0, E1
of every end state at its T1, written as ``E0s_samples_{name}.npy`` / ``E1s_samples_{name}.npy`` (eval_energy.py:86-87) and, with ``logw``
= -(E1 - E0 + dlogp) and ``ess_ti`` (the ESS of the full TI weights; with ``bootstrap`` also ``ess_ti_ci``), added to the npz; ``ess``
keeps its meaning.  The key is checked before the rollout; sample_latent and sample_adw refuse it.  sample_ambient only:
``"zmatrix": {"order": [...], "ref_atoms": [[r1, r2, r3], ...], "bins": 64, "length_range": [lo, hi], "scale": s, "iqr_k": k}`` or, in
place of order / ref_atoms, ``{"bonds": [[i, j], ...], "root": 0, ...}`` (zmatrix.ZMatrix / ZMatrix.from_bonds; bins, length_range,
scale and iqr_k optional; scale defaults to the energy key's, else 1) computes the Z-matrices of every x0 and every end state on the
GPU, coordinates divided by scale as in results_00031.py:173-174, and adds ``torsions_0/1`` [B, A-3], ``bond_angles_0/1`` [B, A-2],
``bond_lengths_0/1`` [B, A-1] (gen_torsions / gen_bond_angles / gen_bond_lengths; 0: x0, 1: the end state), ``zmat_marginals_0/1``
[3A-6, bins] and ``zmat_ranges`` [3A-6, 2] (observables.zmatrix_marginals: lengths, angles, torsions) to the npz.  The x0 are samples
of the source ensemble and stay unweighted; the end state's marginals are weighted by the run's ``logw`` when the energy key supplies
it, and with ``iqr_k`` (which needs the energy key) the reference's filter_iqr(weights, k) mask -- written as ``zmat_keep`` [B] -- is
applied to them.  The key is checked before the rollout; sample_latent and sample_adw refuse it.  sample_latent with ``return_dlogp`` only:
``"bg": {"forcefield": <path>, "scale": <s>}`` (the keys and checks of the energy key) evaluates the Boltzmann-generator weights on the
GPU: per batch E1 of the end state at each molecule's T (observables.ff_energy at to_nm = 1 / scale), log p(z0) of the batch's starting
noise and ``logw_bg`` = -(E1 + log p(z0) + dlogp) (observables.bg_logw, the log of calc_importance_weights); it writes
``E1s_samples_{name}_forward.npy`` and ``bg_{name}_forward.npz`` with ``E1``, ``log_pz``, ``logw_bg``, ``ess_bg`` (gen_ess_bg, k = None)
and, with ``bootstrap``, ``ess_bg_ci`` -- with or without CV descriptors.  sample_ambient: ``"bg": true`` (needs the energy key and a
dataset built with ``use_latent_trajs``) adds to the npz, for the latent -> ambient chain, ``log_pz`` = log p(latent_z), ``logw_bg`` =
-(E1 + log p(latent_z) + latent_dlogp + dlogp), ``ess_bg`` and, with ``bootstrap``, ``ess_bg_ci``.  As in the reference, log p(z0) is
the full 3A-dimensional normal although the noise is centred, and the constant Jacobian of ``scale`` is dropped: both are constants of
a run and cancel in normalised weights and the ESS.  One species per run; the key is checked before the rollout; sample_adw refuses it.
sample_ambient only, next to the zmatrix key (whose topology it uses): ``"tica": {"traj": <.npy as generate_md writes it>, "n_frames":
<frames per replica>, "temperature": T, "lags": [...], "dim": 2, "bins": 80, "range": [lo, hi], "epsilon": 1e-6}`` (traj, n_frames,
temperature and lags required) fits TICA on the (cos, sin)-encoded torsions of that temperature's MD frames at every lag on the GPU
(observables.tica_fit; the replicas are the trajectories; a torsion does not depend on the length unit, so no scale is needed; a NaN
row -- a temperature that was not simulated -- is refused) and adds ``tica_lags``, ``tica_eigenvalues``, ``tica_timescales``,
``tica_rank``, ``tica_mean``, ``tica_components`` and the marginals of the projections [n_lag, dim, bins] ``tica_hist_md`` (the fitted
frames, unweighted), ``tica_hist_0`` (the x0, unweighted), ``tica_hist_1`` (the end state, weighted by the run's ``logw`` and masked by
``zmat_keep`` where those exist) with ``tica_edges`` to the npz.  The key is checked before the rollout; sample_latent and sample_adw
refuse it.
Without the keys exactly the reference's files are written.

  score_checkpoints <- the held-out evaluation of mdqm9/train_ambient.py:153-157, which decides what weights are kept
Scores checkpoints by the velocity loss they were trained on (thermo.losses, on the GPU) and writes ``val_loss_{data_save_name}.npz``.
Keys: ``gamma`` ('brownian' | 'sin2' | 'sig_sum') and ``t_distr`` ('uniform' | 'beta'), the reference's names; optional
``interpolant_a`` (1.0), ``n_draws`` (1), ``center`` ('batch' for molecules; adw is never centred), ``tbins`` (0), ``seed`` (0).

  train_adw <- /root/reference/adw/train.py:18-100   epoch_{k}.npz, train_state.npz, log.npz under model_save_path/model_save_name/
The training loop on the GPU (thermo.adw.Trainer).  Keys of the reference: ``hidden_size``, ``num_layers``, ``lr``, ``wd``,
``batch_size``, ``epochs``, ``a``, ``seed``, ``model_save_path``, ``model_save_name``; of this build, all optional: ``gamma``
('brownian'), ``t_distr`` ('uniform'), ``dim`` (1), ``max_grad_norm`` (1, the reference's clip).  Checkpoints are .npz state dicts in
the reference's keys (fp64), which score_checkpoints reads; torch pickles are not written.

  train_ambient, train_latent <- mdqm9/train_ambient.py:99-176, mdqm9/train_latent.py
  {name}_{epoch}_weights.npz, {name}_best{epoch}_weights.npz, train_state.npz, log.npz under model_save_path/model_save_name/
The molecule training loops on resident arrays (thermo.ambient.Trainer.fit / thermo.latent.Trainer.fit: an epoch's steps in one
device call).  Keys of the reference: ``n_features``, ``score_layers``, ``batch_size``, ``n_epochs``, ``learning_rate``,
``weight_decay``, ``a``, ``gamma``, ``t_distr``, ``seed``, ``align`` (latent), ``model_save_path``, ``model_save_name``; optional
``temp_length`` (10) and ``temperatures``.  The datasets stay with the caller: the sets are (x [n, A, 3], T [n]) arrays.

  generate_md   (no counterpart in the reference: its trajectory files come from its authors)
  {traj_path}/{split}/{traj_filename} per split, {traj_path}/md_log.npz
Langevin dynamics under a force field on the GPU (md.LangevinSampler) into the multi-temperature layout data.load_trajectory reads.
Keys: ``forcefield`` (the XML of an OpenMM System), ``x0`` (.npy [A, 3] or [n, A, 3] starting geometries in model units, used in
turn), ``scale`` or ``to_nm`` (model units per nm as the energy key has it, or nm per model unit), ``temperatures`` (each in
data.TEMPERATURES), ``n_replicas`` (per temperature), ``dt`` (ps), ``friction`` (1/ps), ``n_equil``, ``n_frames``, ``stride``,
``seed``, ``splits`` ({name: fraction of the replicas}), ``traj_path``, ``traj_filename``.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from . import _lib
from . import observables as _obs
from .thermo import adw as _adw
from .thermo import adw_nd as _adw_nd
from .thermo import ambient as _amb
from .thermo import latent as _lat
from .thermo import _common as C
from .thermo import interpolants as _interp
from .thermo import losses as _losses


def load_config(path: str, filename: str, argv=()) -> argparse.Namespace:
    settings = json.load(open(os.path.join(path, filename)))
    parser = argparse.ArgumentParser()
    for key, value in settings.items():
        parser.add_argument(f"--{key}", type=type(value), default=value)
    return parser.parse_args(list(argv))


def _regroup(sample, batch_idx):
    """[n_step, N, 3] -> [B, n_step, A, 3] exactly like ``np.array([sample[:, batch_idx == i] ...])`` (sample_ambient.py:93)."""
    sample, batch_idx = C.to_numpy(sample), C.to_numpy(batch_idx)
    return np.array([sample[:, batch_idx == i] for i in range(int(batch_idx.max()) + 1)])


def _divergence_kw(config):
    return dict(divergence=getattr(config, "divergence", "exact"), n_probes=getattr(config, "n_probes", 1),
                probe_seed=getattr(config, "probe_seed", 0))


def _observe_kw(config):
    o = getattr(config, "observables", None)
    if o is None:
        return {}
    o = dict(o)
    o.pop("bins", None)
    o.pop("bootstrap", None)
    o.pop("gedmd", None)
    o.pop("kinetics", None)
    o.pop("energy", None)
    o.pop("zmatrix", None)
    o.pop("tica", None)
    if o.pop("bg", None) is not None and not o:
        return {}                              # the bg key alone: weights without collective variables, no observer
    if o.get("ref") is not None:
        o["ref"] = np.asarray(o["ref"], np.float32)
    return dict(observe=o)


GEDMD_KEYS = {"p": 50, "sigma": 0.6, "nev": 4, "tol": 1e-4, "n_boot": 1000, "seed": 0, "potential": (4.0, 0.5)}
GEDMD_SOLVER = "host"          # default of the key observables.gedmd.solver: "host" (numpy) or "device" (ti_obs_gedmd_spectrum, p <= 64)


def _gedmd_solver(o):
    """observables["gedmd"]["solver"] checked; the default without the key"""
    g = dict(o).get("gedmd")
    solver = g.get("solver", GEDMD_SOLVER) if isinstance(g, dict) else GEDMD_SOLVER
    if solver not in _obs.SOLVERS:
        raise ValueError(f"observables['gedmd']['solver'] must be one of {_obs.SOLVERS}, got {solver!r}")
    return solver


def _gedmd_settings(o):
    """observables["gedmd"] completed with the defaults above and checked; None without the key."""
    g = dict(o).get("gedmd")
    if g is None:
        return None
    if not isinstance(g, dict) or set(g) - set(GEDMD_KEYS) - {"solver"}:
        raise ValueError(f"observables['gedmd'] must be a dict with keys out of {sorted(GEDMD_KEYS) + ['solver']}, got {g!r}")
    solver = _gedmd_solver(o)
    g = {**GEDMD_KEYS, **{k: v for k, v in g.items() if k != "solver"}}
    for k in ("p", "nev", "n_boot", "seed"):
        if isinstance(g[k], bool) or int(g[k]) != g[k] or int(g[k]) < (0 if k == "seed" else 1):
            raise ValueError(f"observables['gedmd'][{k!r}] must be an integer >= {0 if k == 'seed' else 1}, got {g[k]!r}")
        g[k] = int(g[k])
    if not (np.isfinite(g["sigma"]) and g["sigma"] > 0 and np.isfinite(g["tol"]) and g["tol"] >= 0):
        raise ValueError("observables['gedmd']: sigma must be finite and > 0, tol finite and >= 0")
    pot = tuple(float(v) for v in np.asarray(g["potential"], np.float64).reshape(-1))
    if len(pot) != 2 or not np.isfinite(pot).all():
        raise ValueError(f"observables['gedmd']['potential'] must be [a, b] of U = a (x^2 - 1)^2 + b x, got {g['potential']!r}")
    g["potential"] = pot
    if g["nev"] > g["p"]:
        raise ValueError("observables['gedmd']: nev must not exceed p")
    if solver == "device" and g["p"] > _obs._lib.EIGH_MAX_N:
        raise ValueError(f"observables['gedmd']: solver 'device' takes p <= {_obs._lib.EIGH_MAX_N}")
    return g


def _gedmd_arrays(g, x0, x1, dlogp, beta0, beta1, solver=GEDMD_SOLVER):
    """gedmd_eigenvalues [nev], gedmd_ci [2, nev], gedmd_rank of the end state x1 [B] reweighted to beta1: logw = beta0 U(x0) -
    beta1 U(x1) - dlogp in fp64 (calculate_weights of the reference's reweight_gedmd.py, which hard-codes beta0 = 1), a = 2 / beta1."""
    a, b = g["potential"]
    U = lambda x: a * (x * x - 1.0) ** 2 + b * x
    x0, x1 = np.asarray(x0, np.float64).reshape(-1), np.asarray(x1, np.float64).reshape(-1)
    logw = (float(beta0) * U(x0) - float(beta1) * U(x1) - np.asarray(dlogp, np.float64).reshape(-1)).astype(np.float32)
    omega = _obs.sample_rff_gaussian(1, g["p"], g["sigma"], g["seed"])
    res = _obs.gedmd_generator(x1.astype(np.float32), omega, g["nev"], 2.0 / float(beta1), tol=g["tol"], logw=logw, n_boot=g["n_boot"], seed=g["seed"],
                               solver=solver)
    return dict(gedmd_eigenvalues=res.eigenvalues, gedmd_ci=res.ci, gedmd_rank=np.int64(res.rank))


KINETICS_KEYS = {"columns": None, "p": 300, "sigma": 5.0, "nev": 4, "tol": 1e-4, "n_boot": 1000, "seed": 0, "temperature": None}
KINETICS_KB = 0.008314462618        # kJ / (mol K), the reference's constant (mdqm9/analysis/gedmd.py)
KINETICS_SOLVER = "host"       # default of the key observables.kinetics.solver: "host" (gedmd_generator) or "device" (gedmd_generator_wide)


def _kinetics_solver(o):
    """observables["kinetics"]["solver"] checked; the default without the key"""
    g = dict(o).get("kinetics")
    solver = g.get("solver", KINETICS_SOLVER) if isinstance(g, dict) else KINETICS_SOLVER
    if solver not in _obs.SOLVERS:
        raise ValueError(f"observables['kinetics']['solver'] must be one of {_obs.SOLVERS}, got {solver!r}")
    return solver


def _kinetics_settings(o, K=None):
    """observables["kinetics"] completed with the defaults above and checked (columns against K CV columns when given); None without
    the key."""
    g = dict(o).get("kinetics")
    if g is None:
        return None
    if not isinstance(g, dict) or set(g) - set(KINETICS_KEYS) - {"solver"} or "columns" not in g or "temperature" not in g:
        raise ValueError(f"observables['kinetics'] must be a dict with 'columns', 'temperature' and keys out of {sorted(KINETICS_KEYS) + ['solver']}, got {g!r}")
    _kinetics_solver(o)
    g = {**KINETICS_KEYS, **{k: v for k, v in g.items() if k != "solver"}}
    for k in ("p", "nev", "n_boot", "seed"):
        if isinstance(g[k], bool) or int(g[k]) != g[k] or int(g[k]) < (0 if k == "seed" else 1):
            raise ValueError(f"observables['kinetics'][{k!r}] must be an integer >= {0 if k == 'seed' else 1}, got {g[k]!r}")
        g[k] = int(g[k])
    cols = list(g["columns"]) if isinstance(g["columns"], (list, tuple)) else None
    if not cols or len(cols) > _obs._lib.GRAM_MAX_D or any(isinstance(c, bool) or int(c) != c or int(c) < 0 for c in cols) \
            or (K is not None and max(cols) >= K):
        raise ValueError(f"observables['kinetics']['columns'] must list 1..{_obs._lib.GRAM_MAX_D} CV columns"
                         f"{'' if K is None else f' below {K}'}, got {g['columns']!r}")
    g["columns"] = [int(c) for c in cols]
    if not (np.isfinite(g["sigma"]) and g["sigma"] > 0 and np.isfinite(g["tol"]) and g["tol"] >= 0):
        raise ValueError("observables['kinetics']: sigma must be finite and > 0, tol finite and >= 0")
    if isinstance(g["temperature"], bool) or not (np.isfinite(g["temperature"]) and g["temperature"] > 0):
        raise ValueError(f"observables['kinetics']['temperature'] must be finite and > 0, got {g['temperature']!r}")
    if g["p"] > _obs._lib.GRAM_WIDE_MAX_P or g["nev"] > g["p"]:
        raise ValueError(f"observables['kinetics']: p must not exceed {_obs._lib.GRAM_WIDE_MAX_P} and nev must not exceed p")
    return g


def _check_kinetics(config, molecules=True):
    """Before the rollout, so that a slip in the key does not cost the run: observables["kinetics"] validated against the descriptor
    count (sample_ambient / sample_latent), refused in sample_adw (molecules=False), whose analysis is the `gedmd` key."""
    o = getattr(config, "observables", None)
    if o is None or dict(o).get("kinetics") is None:
        return
    if not molecules:
        raise ValueError("observables['kinetics'] is for sample_ambient / sample_latent (torsion columns, unweighted); sample_adw takes "
                         "observables['gedmd']")
    _kinetics_settings(o, len(dict(o)["descriptors"]))


def _kinetics_arrays(g, cv_end, solver=KINETICS_SOLVER):
    """kinetics_eigenvalues [nev], kinetics_ci [2, nev], kinetics_rank of the selected columns of the end-state CVs cv_end [B, K]:
    the unweighted generator spectrum of the reference's mdqm9/analysis/gedmd.py, a = k_B T.  solver "device": the same arguments to
    observables.gedmd_generator_wide, the p x p algebra on the GPU as well."""
    x = np.ascontiguousarray(cv_end[:, g["columns"]], np.float32)
    omega = _obs.sample_rff_gaussian(x.shape[1], g["p"], g["sigma"], g["seed"])
    generator = _obs.gedmd_generator_wide if solver == "device" else _obs.gedmd_generator
    res = generator(x, omega, g["nev"], KINETICS_KB * float(g["temperature"]), tol=g["tol"], n_boot=g["n_boot"], seed=g["seed"])
    return dict(kinetics_eigenvalues=res.eigenvalues, kinetics_ci=res.ci, kinetics_rank=np.int64(res.rank))


ENERGY_KEYS = ("forcefield", "scale")


def _check_energy(config, driver="sample_ambient"):
    """Before the rollout: observables["energy"] validated and its force field read (sample_ambient) -> (ForceField, to_nm), None
    without the key; refused by the other two drivers, whose weights it cannot complete."""
    o = getattr(config, "observables", None)
    g = None if o is None else dict(o).get("energy")
    if g is None:
        return None
    if driver == "sample_latent":
        raise ValueError("observables['energy'] is for sample_ambient: the latent map's weights also need log p(z0) of the prior "
                         "(calc_importance_weights), which is not evaluated here; observables['bg'] evaluates both")
    if driver == "sample_adw":
        raise ValueError("observables['energy'] is for sample_ambient: it evaluates a molecular force field; the double well's potential "
                         "enters through observables['gedmd']['potential']")
    if not isinstance(g, dict) or set(g) != set(ENERGY_KEYS):
        raise ValueError(f"observables['energy'] must be a dict with exactly the keys {list(ENERGY_KEYS)}, got {g!r}")
    scale = g["scale"]
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"observables['energy']['scale'] must be finite and > 0, got {scale!r}")
    if not bool(getattr(config, "return_dlogp", False)):
        raise ValueError("observables['energy'] needs return_dlogp: the TI weights are exp(-(E1 - E0 + dlogp))")
    from . import forcefield as _ff
    return _ff.ForceField.from_openmm_xml(os.fspath(g["forcefield"])), 1.0 / float(scale)


def _check_bg(config, driver, dataset=None):
    """Before the rollout: observables["bg"] validated; None without the key.  sample_latent: a dict with the keys of the energy key
    and their checks -> (ForceField, to_nm).  sample_ambient: true, with the energy key and a dataset built with use_latent_trajs
    (else latent_z is the zero placeholder) -> True.  sample_adw refuses it."""
    o = getattr(config, "observables", None)
    g = None if o is None else dict(o).get("bg")
    if g is None or (g is False and driver == "sample_ambient"):
        return None
    if driver == "sample_adw":
        raise ValueError("observables['bg'] is for sample_latent / sample_ambient: it weights molecules by a force field and the normal "
                         "prior; the double well's potential enters through observables['gedmd']['potential']")
    if driver == "sample_ambient":
        if g is not True:
            raise ValueError(f"observables['bg'] must be true in sample_ambient (the force field is the energy key's), got {g!r}")
        if dict(o).get("energy") is None:
            raise ValueError("observables['bg'] needs observables['energy'] in sample_ambient: the chain's weights are "
                             "exp(-(E1 + log p(z0) + latent_dlogp + dlogp))")
        if "descriptors" not in dict(o):
            raise ValueError("observables['bg'] adds to the observables npz in sample_ambient, which needs observables['descriptors']")
        if not getattr(dataset, "use_latent_trajs", False):
            raise ValueError("observables['bg'] needs a dataset built with use_latent_trajs: without it latent_z is the zero placeholder, "
                             "not the noise the chain started from")
        return True
    if not isinstance(g, dict) or set(g) != set(ENERGY_KEYS):
        raise ValueError(f"observables['bg'] must be a dict with exactly the keys {list(ENERGY_KEYS)}, got {g!r}")
    scale = g["scale"]
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"observables['bg']['scale'] must be finite and > 0, got {scale!r}")
    if not bool(getattr(config, "return_dlogp", False)):
        raise ValueError("observables['bg'] needs return_dlogp: the weights are exp(-(E1 + log p(z0) + dlogp))")
    from . import forcefield as _ff
    return _ff.ForceField.from_openmm_xml(os.fspath(g["forcefield"])), 1.0 / float(scale)


def _batch_bg(b, batch, sample, ff, to_nm):
    """(E1, z0) of one sample_latent batch: the reduced energies [B] float64 of the end state at every molecule's T, and the noise
    [B, A, 3] float32 the batch started from"""
    from .thermo import _molecule as _mol
    sb = _mol.split_species_batch(batch, b.ATOM_KEY)
    if sb.n_atoms is not None:
        raise ValueError("observables['bg'] takes one species per run (one force field)")
    if not hasattr(batch, "T"):
        raise ValueError("observables['bg'] needs the batch's temperatures (batch.T): the energies are reduced by R T")
    B, A = sb.B, sb.A
    eng = b.engine_of(sb)
    eng.set_forcefield(ff)
    x1 = C.as_f32(sample[-1], (B, A, 3))
    T = C.as_f32(batch.T, (B, A))[:, 0]
    T = T.contiguous() if C.is_cuda(x1) else np.ascontiguousarray(T)
    return C.to_numpy(eng.ff_energy(x1, to_nm, T)), np.ascontiguousarray(C.to_numpy(C.as_f32(batch.x0, (B, A, 3))))


def _bg_arrays(config, z0, E1, nd_bg, nd_ti=None):
    """log_pz, logw_bg, ess_bg (and ess_bg_ci with the bootstrap key) of a run's prior samples z0 [B, A, 3], reduced end-state energies
    and end-state dlogps (nd_ti: the ambient map's, on a latent -> ambient chain)"""
    z0 = np.ascontiguousarray(z0, np.float32)
    logw = _obs.bg_logw(z0, E1, nd_bg, nd_ti)
    _obs.importance_weights(logw)                  # refuses a non-finite log-weight by index, as every consumer of logw_bg would
    ess = _obs.ess_bg(z0, E1, nd_bg, nd_ti, n_boot=0).point
    out = dict(log_pz=_obs.log_prior(z0), logw_bg=logw, ess_bg=np.float64(ess))
    n_boot = dict(config.observables).get("bootstrap")
    if n_boot is not None:
        if isinstance(n_boot, bool) or int(n_boot) != n_boot or int(n_boot) < 1:
            raise ValueError(f"observables['bootstrap'] must be an integer >= 1, got {n_boot!r}")
        out["ess_bg_ci"] = np.asarray(_obs.ess_bg(z0, E1, nd_bg, nd_ti, n_boot=int(n_boot)).ci, np.float64)
    return out


def _batch_energies(b, batch, sample, ff, to_nm):
    """(E0, E1) [B] float64 of one batch: the reduced energies of x0 at every molecule's T0 and of the end state at its T1"""
    from .thermo import _molecule as _mol
    sb = _mol.split_species_batch(batch, b.ATOM_KEY)
    if sb.n_atoms is not None:
        raise ValueError("observables['energy'] takes one species per run (one force field)")
    B, A = sb.B, sb.A
    eng = b.engine_of(sb)
    eng.set_forcefield(ff)
    x0 = C.as_f32(batch.x0, (B, A, 3))
    x1 = C.as_f32(sample[-1], (B, A, 3))
    per_mol = lambda v: C.as_f32(v, (B, A))[:, 0]
    T0, T1 = per_mol(batch.T0), per_mol(batch.T1)
    if C.is_cuda(x0):
        T0, T1 = T0.contiguous(), T1.contiguous()
    else:
        T0, T1 = np.ascontiguousarray(T0), np.ascontiguousarray(T1)
    return C.to_numpy(eng.ff_energy(x0, to_nm, T0)), C.to_numpy(eng.ff_energy(x1, to_nm, T1))


def _energy_arrays(config, E0, E1, dl):
    """E0, E1, logw, ess_ti (and ess_ti_ci with the bootstrap key) of a run's reduced energies and end-state dlogp"""
    logw = _obs.ti_logw(E0, E1, dl)
    _, ess = _obs.importance_weights(logw)
    out = dict(E0=E0, E1=E1, logw=logw, ess_ti=np.float64(ess))
    n_boot = dict(config.observables).get("bootstrap")
    if n_boot is not None:
        out["ess_ti_ci"] = np.asarray(_obs.ess_ti(E0, E1, dl, n_boot=int(n_boot)).ci, np.float64)
    return out


ZMATRIX_KEYS = ("order", "ref_atoms", "bonds", "root", "bins", "length_range", "scale", "iqr_k")


def _check_zmatrix(config, driver="sample_ambient"):
    """Before the rollout: observables["zmatrix"] validated (sample_ambient) -> dict(zm, bins, length_range, scale, iqr_k), None
    without the key; refused by the other two drivers."""
    o = getattr(config, "observables", None)
    g = None if o is None else dict(o).get("zmatrix")
    if g is None:
        return None
    if driver != "sample_ambient":
        raise ValueError(f"observables['zmatrix'] is for sample_ambient (molecules in Cartesian coordinates with a fixed topology); "
                         f"{driver} does not take it")
    from . import zmatrix as _zm
    if not isinstance(g, dict) or set(g) - set(ZMATRIX_KEYS):
        raise ValueError(f"observables['zmatrix'] must be a dict with keys out of {list(ZMATRIX_KEYS)}, got {g!r}")
    explicit, bonded = "ref_atoms" in g, "bonds" in g
    if explicit == bonded or (bonded and "order" in g) or (explicit and "root" in g):
        raise ValueError("observables['zmatrix'] takes either 'ref_atoms' (with an optional 'order') or 'bonds' (with an optional 'root')")
    try:
        if explicit:
            zm = _zm.ZMatrix(g.get("order"), np.asarray(g["ref_atoms"]))
        else:
            bonds = np.asarray(g["bonds"])
            if bonds.ndim != 2 or bonds.shape[1:] != (2,) or bonds.dtype.kind not in "iu" or bonds.size == 0:
                raise ValueError("bonds must be a non-empty integer list [[i, j], ...]")
            zm = _zm.ZMatrix.from_bonds(bonds, int(bonds.max()) + 1, g.get("root", 0))
        bins, lo, hi = _obs.check_bins(g.get("bins", 64), g.get("length_range", (0.0, 4.0)))
    except (ValueError, TypeError) as e:
        raise ValueError(f"observables['zmatrix']: {e}") from None
    energy = dict(o).get("energy")
    scale = g.get("scale", energy["scale"] if isinstance(energy, dict) and "scale" in energy else 1.0)
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"observables['zmatrix']['scale'] must be finite and > 0, got {scale!r}")
    k = g.get("iqr_k")
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)) or not (np.isfinite(k) and k > 0):
            raise ValueError(f"observables['zmatrix']['iqr_k'] must be finite and > 0, got {k!r}")
        if energy is None:
            raise ValueError("observables['zmatrix']['iqr_k'] filters on the TI weights: it needs observables['energy']")
    return dict(zm=zm, bins=bins, length_range=(lo, hi), scale=float(scale), iqr_k=None if k is None else float(k))


def _batch_zmatrices(b, batch, sample, g):
    """(z0, z1) [B, A-1, 3] float32 of one batch: the Z-matrices of x0 and of the end state, coordinates divided by the scale"""
    from .thermo import _molecule as _mol
    sb = _mol.split_species_batch(batch, b.ATOM_KEY)
    if sb.n_atoms is not None:
        raise ValueError("observables['zmatrix'] takes one species per run (one topology)")
    B, A = sb.B, sb.A
    if A != g["zm"].A:
        raise ValueError(f"observables['zmatrix'] describes {g['zm'].A} atoms, the molecules have {A}")
    eng = b.engine_of(sb)
    out = []
    for x in (batch.x0, sample[-1]):
        x = np.ascontiguousarray(C.to_numpy(C.as_f32(x, (B, A, 3)))) / g["scale"]        # fp32 / python float: fp32, as the reference divides
        out.append(_obs.zmatrix(eng, np.ascontiguousarray(x, np.float32), g["zm"]))
    return out[0], out[1]


def _zmatrix_arrays(g, z0, z1, logw):
    """The arrays the zmatrix key adds; logw [B] float32 of the energy key or None"""
    keep = None if g["iqr_k"] is None else _obs.iqr_keep(logw, g["iqr_k"])
    m0 = _obs.zmatrix_marginals(z0, None, None, g["bins"], g["length_range"])
    m1 = _obs.zmatrix_marginals(z1, logw, keep, g["bins"], g["length_range"])
    out = dict(torsions_0=_obs.torsions(z0), torsions_1=_obs.torsions(z1), bond_angles_0=_obs.bond_angles(z0),
               bond_angles_1=_obs.bond_angles(z1), bond_lengths_0=_obs.bond_lengths(z0), bond_lengths_1=_obs.bond_lengths(z1),
               zmat_marginals_0=m0.hist, zmat_marginals_1=m1.hist, zmat_ranges=m0.ranges)
    if keep is not None:
        out["zmat_keep"] = keep
    return out


TICA_KEYS = {"traj": None, "n_frames": None, "temperature": None, "lags": None, "dim": 2, "bins": 80, "range": (-2.5, 2.5), "epsilon": 1e-6}


def _check_tica(config, driver="sample_ambient"):
    """Before the rollout: observables["tica"] validated (sample_ambient) -> dict(frames [m, A, 3] float32 of the temperature,
    traj_off, lags, dim, bins, range, epsilon), None without the key; refused by the other two drivers."""
    o = getattr(config, "observables", None)
    g = None if o is None else dict(o).get("tica")
    if g is None:
        return None
    if driver != "sample_ambient":
        raise ValueError(f"observables['tica'] is for sample_ambient (it fits on the torsions of an MD trajectory of the species); "
                         f"{driver} does not take it")
    from . import data as _data
    required = [k for k, v in TICA_KEYS.items() if v is None]
    if not isinstance(g, dict) or set(g) - set(TICA_KEYS) or any(k not in g for k in required):
        raise ValueError(f"observables['tica'] must be a dict with the keys {required} and optionally "
                         f"{[k for k in TICA_KEYS if k not in required]}, got {g!r}")
    if dict(o).get("zmatrix") is None:
        raise ValueError("observables['tica'] needs observables['zmatrix']: the torsions are those of its topology")
    if dict(o).get("descriptors") is None:
        raise ValueError("observables['tica'] adds to the observables npz, which needs observables['descriptors']")
    nf, T = g["n_frames"], g["temperature"]
    if isinstance(nf, bool) or not isinstance(nf, (int, np.integer)) or nf < 1:
        raise ValueError(f"observables['tica']['n_frames'] must be an integer >= 1, got {nf!r}")
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or int(T) not in _data.TEMPERATURES:
        raise ValueError(f"observables['tica']['temperature'] must be one of {list(_data.TEMPERATURES)}, got {T!r}")
    lags = np.asarray(g["lags"])
    if lags.ndim != 1 or lags.size < 1 or lags.dtype.kind not in "iu" or np.any(lags < 1) or np.any(lags >= int(nf)):
        raise ValueError(f"observables['tica']['lags'] must be a list of integers in 1..n_frames - 1, got {g['lags']!r}")
    dim, eps = g.get("dim", 2), g.get("epsilon", 1e-6)
    if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or dim < 1:
        raise ValueError(f"observables['tica']['dim'] must be an integer >= 1, got {dim!r}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not (np.isfinite(eps) and eps >= 0):
        raise ValueError(f"observables['tica']['epsilon'] must be finite and >= 0, got {eps!r}")
    try:
        bins, lo, hi = _obs.check_bins(g.get("bins", 80), g.get("range", (-2.5, 2.5)))
    except (ValueError, TypeError) as e:
        raise ValueError(f"observables['tica']: {e}") from None
    try:
        traj = np.load(os.fspath(g["traj"]), mmap_mode="r")
    except (OSError, ValueError, TypeError) as e:
        raise ValueError(f"observables['tica']['traj']: {e}") from None
    if traj.ndim != 4 or traj.shape[0] != len(_data.TEMPERATURES) or traj.shape[3] != 3 or traj.shape[1] < 1 or traj.shape[1] % int(nf):
        raise ValueError(f"observables['tica']['traj'] must hold [{len(_data.TEMPERATURES)}, n_replicas * n_frames, A, 3] with n_frames = {nf}, "
                         f"got {traj.shape}")
    frames = np.ascontiguousarray(traj[_data.TEMPERATURES.index(int(T))], np.float32)
    if not np.isfinite(frames).all():
        raise ValueError(f"observables['tica']: the frames at {T} K are not finite (a temperature that was not simulated is a NaN row)")
    A = frames.shape[1]
    if not 4 <= A <= _lib.TICA_MAX_K + 3:
        raise ValueError(f"observables['tica'] takes molecules of 4..{_lib.TICA_MAX_K + 3} atoms (1..{_lib.TICA_MAX_K} torsions), got {A}")
    if lags.size > _lib.TICA_MAX_LAGS:
        raise ValueError(f"observables['tica']['lags'] takes at most {_lib.TICA_MAX_LAGS} lags, got {lags.size}")
    if int(dim) > 2 * (A - 3):
        raise ValueError(f"observables['tica']['dim'] must be <= {2 * (A - 3)} (two features per torsion), got {dim}")
    return dict(frames=frames, traj_off=np.arange(0, frames.shape[0] + 1, int(nf), dtype=np.int64), lags=lags.astype(np.int32), dim=int(dim),
                bins=bins, range=(lo, hi), epsilon=float(eps))


def _tica_md_zmatrix(b, batch, t, zmat):
    """z [m, A-1, 3] of the MD frames the tica key fits on, on the engine of the batch's species.  A torsion does not depend on the
    length unit, so the frames are taken as they are."""
    from .thermo import _molecule as _mol
    sb = _mol.split_species_batch(batch, b.ATOM_KEY)
    return _obs.zmatrix(b.engine_of(sb), t["frames"], zmat["zm"])


def _tica_arrays(t, z_md, z0, z1, logw, keep):
    """The arrays the tica key adds: the model fitted on the torsions of the MD frames and the marginals of the projected MD frames, x0
    and end state (the latter weighted by logw [B] float32 and masked by keep [B] uint8 where they exist)"""
    tor = lambda z: _obs.torsions(C.to_numpy(z))                    # the strided view z[:, 2:, 2]: read in place, no copy
    m = _obs.tica_fit(tor(z_md), t["traj_off"], t["lags"], dim=t["dim"], epsilon=t["epsilon"])
    kw = dict(bins=t["bins"], range=t["range"])
    h_md, h_0, h_1 = (_obs.tica_marginals(m, tor(z), lw, kp, **kw) for z, lw, kp in ((z_md, None, None), (z0, None, None), (z1, logw, keep)))
    return dict(tica_lags=m.lags, tica_eigenvalues=m.eigenvalues, tica_timescales=m.timescales, tica_rank=m.rank, tica_mean=m.mean,
                tica_components=m.components, tica_hist_md=h_md.hist, tica_hist_0=h_0.hist, tica_hist_1=h_1.hist, tica_edges=h_md.edges)


def _write_observables(config, path, cvs, dlogps, gedmd=None, energy=None, zmat=None, bg=None, tica=None):
    """cvs: per-batch [rows, B_i, K]; dlogps: per-batch end-state [B_i] (empty without return_dlogp); gedmd: (x0, x1, beta0, beta1)
    of an adw run whose observables carry the gedmd key; energy: (E0, E1) [B] of a run with the energy key; bg: (latent_z [B, A, 3],
    latent_dlogp [B]) of a sample_ambient run with the bg key; tica: (settings, z [m, A-1, 3] of the MD frames) of a sample_ambient run
    with the tica key"""
    cv = np.concatenate([C.to_numpy(c) for c in cvs], axis=1).astype(np.float32)
    dl = np.concatenate([np.asarray(d, np.float32).reshape(-1) for d in dlogps]) if dlogps else None
    hist, edges, ess = _obs.end_state_summary(np.ascontiguousarray(cv[-1]), dl, bins=int(dict(config.observables).get("bins", 32)))
    extra = {}
    n_boot = dict(config.observables).get("bootstrap")
    if n_boot is not None:                     # the ESS with its 95 % bootstrap interval (observables.bootstrap; B without weights)
        if isinstance(n_boot, bool) or int(n_boot) != n_boot or int(n_boot) < 1:
            raise ValueError(f"observables['bootstrap'] must be an integer >= 1, got {n_boot!r}")
        B = cv.shape[1]
        res = _obs.bootstrap(-dl if dl is not None else np.zeros(B, np.float32), "ess", n_boot=int(n_boot))
        extra = dict(ess_ci=np.asarray(res.ci, np.float64), ess_boot=res.estimates)
    g = _gedmd_settings(config.observables)
    if g is not None:
        if gedmd is None or dl is None:
            raise ValueError("observables['gedmd'] is for sample_adw with return_dlogp: the weights need the end-state dlogp")
        extra.update(_gedmd_arrays(g, gedmd[0], gedmd[1], dl, gedmd[2], gedmd[3], solver=_gedmd_solver(config.observables)))
    k = _kinetics_settings(config.observables, cv.shape[2])
    if k is not None:
        extra.update(_kinetics_arrays(k, cv[-1], solver=_kinetics_solver(config.observables)))
    if energy is not None:
        extra.update(_energy_arrays(config, energy[0], energy[1], dl))
        if bg is not None:                     # (latent_z, latent_dlogp) of a chained run with the bg key
            extra.update(_bg_arrays(config, bg[0], energy[1], bg[1], dl))
    if zmat is not None:                       # (settings, z0, z1) of a run with the zmatrix key
        extra.update(_zmatrix_arrays(zmat[0], zmat[1], zmat[2], extra.get("logw")))
        if tica is not None:
            extra.update(_tica_arrays(tica[0], tica[1], zmat[1], zmat[2], extra.get("logw"), extra.get("zmat_keep")))
    np.savez(path, cv=cv, hist=hist, edges=edges, ess=np.float64(ess), **extra)


def sample_ambient(config, b, dataset):
    _check_kinetics(config)
    energy, E0s, E1s = _check_energy(config), [], []
    zmat, z0s, z1s = _check_zmatrix(config), [], []
    tica, z_md = _check_tica(config), None
    if tica is not None and tica["frames"].shape[1] != zmat["zm"].A:
        raise ValueError(f"observables['tica']['traj'] holds {tica['frames'].shape[1]} atoms, the zmatrix key describes {zmat['zm'].A}")
    bg = _check_bg(config, "sample_ambient", dataset)
    os.makedirs(config.data_save_path, exist_ok=True)
    integrator = _amb.MoleculeIntegrator(b=b, method=getattr(config, "method", "dopri5"), rtol=config.rtol, atol=config.atol,
                                         n_step=config.n_steps, return_dlogp=bool(config.return_dlogp), reverse_ode=False,
                                         save_every=getattr(config, "save_every", 1), step_control=getattr(config, "step_control", "batch"),
                                         **_divergence_kw(config), **_observe_kw(config))
    hutch, traj, cvs = integrator.divergence == "hutchinson", 0, []
    latent_noises, latent_dlogps, samples, dlogps, n_fevals = [], [], [], [], 0
    b.eval()
    for batch in dataset.batches(config.batch_size, shuffle=True, seed=config.seed):
        bidx = batch.batch
        latent_noises.append(np.array([batch.latent_z[bidx == i] for i in range(int(bidx.max()) + 1)]))
        latent_dlogps.append(batch.latent_dlogp)
        sample, dlogp, n_fevals, _ = integrator.rollout(batch, traj) if hutch else integrator.rollout(batch)
        traj += int(C.to_numpy(bidx).max()) + 1
        samples.append(_regroup(sample, bidx))
        if config.return_dlogp:
            dlogps.append(C.to_numpy(dlogp)[-1, :])
        if integrator.observe is not None:
            cvs.append(integrator.cv)
        if energy is not None:
            E0, E1 = _batch_energies(b, batch, sample, *energy)
            E0s.append(E0); E1s.append(E1)
        if zmat is not None:
            z0, z1 = _batch_zmatrices(b, batch, sample, zmat)
            z0s.append(z0); z1s.append(z1)
            if tica is not None and z_md is None:
                z_md = _tica_md_zmatrix(b, batch, tica, zmat)
    name = config.data_save_name
    if energy is not None:
        energy = (np.concatenate(E0s), np.concatenate(E1s))
        np.save(os.path.join(config.data_save_path, f"E0s_samples_{name}.npy"), energy[0])
        np.save(os.path.join(config.data_save_path, f"E1s_samples_{name}.npy"), energy[1])
    if cvs:
        _write_observables(config, os.path.join(config.data_save_path, f"observables_{name}.npz"), cvs, dlogps, energy=energy,
                           zmat=None if zmat is None else (zmat, np.concatenate(z0s), np.concatenate(z1s)),
                           bg=None if bg is None else (np.concatenate(latent_noises, axis=0), np.concatenate(latent_dlogps, axis=0)),
                           tica=None if tica is None else (tica, z_md))
    np.save(os.path.join(config.data_save_path, f"latent_noises_{name}.npy"), np.concatenate(latent_noises, axis=0))
    np.save(os.path.join(config.data_save_path, f"latent_dlogps_{name}.npy"), np.concatenate(latent_dlogps, axis=0))
    np.save(os.path.join(config.data_save_path, f"samples_{name}.npy"), np.concatenate(samples, axis=0))
    if config.return_dlogp:
        np.save(os.path.join(config.data_save_path, f"dlogps_{name}.npy"), np.concatenate(dlogps, axis=0))
    return np.concatenate(samples, axis=0), n_fevals


def sample_latent(config, b, dataset):
    _check_kinetics(config)
    _check_energy(config, "sample_latent")
    _check_zmatrix(config, "sample_latent")
    _check_tica(config, "sample_latent")
    bg, E1s, z0s = _check_bg(config, "sample_latent"), [], []
    os.makedirs(config.data_save_path, exist_ok=True)
    integrator = _lat.MoleculeIntegrator(b=b, method=getattr(config, "method", "dopri5"), rtol=config.rtol, atol=config.atol,
                                         n_step=config.n_steps, return_dlogp=bool(config.return_dlogp), reverse_ode=False,
                                         save_every=getattr(config, "save_every", 1), step_control=getattr(config, "step_control", "batch"),
                                         **_divergence_kw(config), **_observe_kw(config))
    hutch, traj, cvs = integrator.divergence == "hutchinson", 0, []
    samples, dlogps = [], []
    b.eval()
    for batch in dataset.batches(config.batch_size, seed=config.seed, drop_last=True):
        sample, dlogp, bidx = integrator.rollout(batch, traj) if hutch else integrator.rollout(batch)
        traj += int(C.to_numpy(bidx).max()) + 1
        samples.append(_regroup(sample, bidx))
        if config.return_dlogp:
            dlogps.append(C.to_numpy(dlogp)[-1, :])                     # sample_latent.py:76-77
        if integrator.observe is not None:
            cvs.append(integrator.cv)
        if bg is not None:
            E1, z0 = _batch_bg(b, batch, sample, *bg)
            E1s.append(E1); z0s.append(z0)
    if cvs:
        _write_observables(config, os.path.join(config.data_save_path, f"observables_{config.data_save_name}_forward.npz"), cvs, dlogps)
    if bg is not None:
        E1 = np.concatenate(E1s)
        np.save(os.path.join(config.data_save_path, f"E1s_samples_{config.data_save_name}_forward.npy"), E1)
        np.savez(os.path.join(config.data_save_path, f"bg_{config.data_save_name}_forward.npz"), E1=E1,
                 **_bg_arrays(config, np.concatenate(z0s), E1, np.concatenate(dlogps, axis=0)))
    out = np.concatenate(samples, axis=0)
    np.save(os.path.join(config.data_save_path, f"samples_{config.data_save_name}_forward.npy"), out)
    if config.return_dlogp:
        np.save(os.path.join(config.data_save_path, f"dlogps_{config.data_save_name}_forward.npy"), np.concatenate(dlogps, axis=0))
    return out


def sample_adw(config, b, x0s_batches):
    """`x0s_batches`: iterable of (x0s [B,1], beta0s [B,1]) like the reference's test loader (adw/sample.py:41-43)."""
    if getattr(b, "dim", 1) != 1:
        raise NotImplementedError(f"sample_adw writes the 1-D double well's samples (component 0, adw/sample.py:59); "
                                  f"a d = {b.dim} model would lose coordinates: use StandardIntegrator.rollout directly")
    assert len(config.beta0s) == len(config.beta1s) == 1            # adw/sample.py:24
    _check_kinetics(config, molecules=False)
    _check_energy(config, "sample_adw")
    _check_zmatrix(config, "sample_adw")
    _check_tica(config, "sample_adw")
    _check_bg(config, "sample_adw")
    integrator = _adw.StandardIntegrator(b=b, method=getattr(config, "method", None) or config.solver_type, rtol=config.rtol,
                                         atol=config.atol, n_step=config.n_step, return_dlogp=bool(config.return_dlogp),
                                         step_control=getattr(config, "step_control", "batch"), fused=bool(getattr(config, "fused", False)),
                                         **_observe_kw(config))
    initial, samples, dlogps, cvs = [], [], [], []
    b.eval()
    for x0s, beta0s in x0s_batches:
        beta1s = np.ones_like(C.to_numpy(beta0s)) * config.beta1s[0]
        sample, dlogp = integrator.rollout(x0s, beta0s=beta0s, beta1s=beta1s)
        initial.append(C.to_numpy(x0s))
        samples.append(C.to_numpy(sample))
        if config.return_dlogp:
            dlogps.append(C.to_numpy(dlogp))
        if integrator.observe is not None:
            cvs.append(integrator.cv)
    out_dir = os.path.join(config.data_save_path, config.model_save_name, f"beta_{config.beta0s[0]}_to_{config.beta1s[0]}")
    os.makedirs(out_dir, exist_ok=True)
    initial = np.array(initial)[:, :, 0].flatten()
    np.save(os.path.join(out_dir, f"initial_samples_epoch_{config.sampling_epoch}.npy"), initial)

    def by_step(chunks):                                             # [n_batches, n_step, B, 1] -> [n_step, n_batches*B]
        arr = np.array(chunks)
        return np.array([arr[:, i, :, 0].flatten() for i in range(arr.shape[1])])

    samples = by_step(samples)
    np.save(os.path.join(out_dir, f"samples_epoch_{config.sampling_epoch}.npy"), samples)
    if config.return_dlogp:
        np.save(os.path.join(out_dir, f"dlogps_epoch_{config.sampling_epoch}.npy"), by_step(dlogps))
    if cvs:
        _write_observables(config, os.path.join(out_dir, f"observables_epoch_{config.sampling_epoch}.npz"), cvs,
                           [d[-1] for d in dlogps] if config.return_dlogp else [],
                           gedmd=(initial, samples[-1], config.beta0s[0], config.beta1s[0]))
    return initial, samples


def _vloss_settings(config):
    """The velocity-loss keys of a config, checked (ValueError) before any device work"""
    g = lambda k, d: getattr(config, k, d)
    gamma, t_distr, center = g("gamma", "brownian"), g("t_distr", "uniform"), g("center", None)
    if gamma not in _interp.GAMMAS:
        raise ValueError(f"config.gamma must be one of {_interp.GAMMAS}, got {gamma!r}")
    if t_distr not in ("uniform", "beta"):
        raise ValueError(f"config.t_distr must be 'uniform' or 'beta', got {t_distr!r}")
    if center not in (None, "batch", "molecule", "none"):
        raise ValueError(f"config.center must be 'batch', 'molecule' or 'none', got {center!r}")
    a, n_draws, tbins, seed = g("interpolant_a", 1.0), g("n_draws", 1), g("tbins", 0), g("seed", 0)
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not np.isfinite(a) or a <= 0:
        raise ValueError(f"config.interpolant_a must be a finite number > 0, got {a!r}")
    for key, v, lo, hi in (("n_draws", n_draws, 1, 1 << 20), ("tbins", tbins, 0, 1024), ("seed", seed, 0, (1 << 64) - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"config.{key} must be an integer in {lo}..{hi}, got {v!r}")
    for key in ("data_save_path", "data_save_name"):
        if not isinstance(g(key, None), str) or not g(key, None):
            raise ValueError(f"config.{key} must be a non-empty string")
    return dict(gamma=gamma, t_distr=t_distr, center=center, a=float(a), n_draws=int(n_draws), tbins=int(tbins), seed=int(seed))


def _load_state_dict(ck):
    """A checkpoint: a state dict, the path of an .npz of one, or the path of a torch file (a state dict or a module)"""
    if isinstance(ck, dict):
        return ck
    if str(ck).endswith(".npz"):
        with np.load(ck) as f:
            return {k: f[k] for k in f.files}
    import torch                                  # the one place torch is needed: the reference saves checkpoints with torch.save
    obj = torch.load(ck, map_location="cpu")
    return obj.state_dict() if hasattr(obj, "state_dict") else obj


def score_checkpoints(config, b, pairs, checkpoints):
    """Velocity loss (StandardVelocityLoss with LinearInterpolant(interpolant_a, gamma)) of every checkpoint on the held-out `pairs`:
    (batch0, batch1) per item for an ambient model, (x0s, x1s, beta0s, beta1s) for adw.  Every checkpoint sees the same (t, z): draw
    d of a pair uses seed = config.seed, draw = d and the pair's running molecule offset.  Writes and returns ``mean`` [K] (per atom
    row for molecules, per particle for adw), ``sem`` [K] (standard error over molecules of their draw-averaged losses), ``tbins``
    [K, n, 2] (sum of the per-molecule losses and count per bin of t) and ``best`` (index of the smallest mean)."""
    s = _vloss_settings(config)
    pairs = [tuple(p) for p in pairs]
    checkpoints = list(checkpoints)
    if not pairs or not checkpoints:
        raise ValueError("score_checkpoints needs at least one pair and one checkpoint")
    if any(len(p) not in (2, 4) or len(p) != len(pairs[0]) for p in pairs):
        raise ValueError("pairs must all be (batch0, batch1) or all (x0s, x1s, beta0s, beta1s)")
    form = len(pairs[0])
    loss_fn = _losses.StandardVelocityLoss(_interp.LinearInterpolant(s["a"], s["gamma"]), s["t_distr"])
    K, n = len(checkpoints), s["tbins"]
    mean, sem, tb = np.zeros(K), np.zeros(K), np.zeros((K, n, 2))
    b.eval()
    for k, ck in enumerate(checkpoints):
        b.load_state_dict(_load_state_dict(ck))
        per_mol, offset = [], 0
        for p in pairs:
            acc = None
            for d in range(s["n_draws"]):
                kw = dict(seed=s["seed"], draw=d, traj_offset=offset, tbins=n, center=s["center"])
                loss_fn(b, *p, **kw) if form == 4 else loss_fn(*p, b, **kw)
                last = loss_fn.last
                l = C.to_numpy(last["loss"]).astype(np.float64)
                acc = l if acc is None else acc + l
                if n:
                    tb[k] += last["tbins"]
            rows_per = last["rows"] // acc.size                      # A for molecules, 1 for adw: the mean is per atom row
            per_mol.append(acc / (s["n_draws"] * rows_per))
            offset += acc.size
        v = np.concatenate(per_mol)
        mean[k] = v.mean()
        sem[k] = v.std(ddof=1) / np.sqrt(v.size) if v.size > 1 else 0.0
    out = dict(mean=mean, sem=sem, tbins=tb, best=np.int64(np.argmin(mean)))
    os.makedirs(config.data_save_path, exist_ok=True)
    np.savez(os.path.join(config.data_save_path, f"val_loss_{config.data_save_name}.npz"), **out)
    return out


class _Plateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(factor, patience) on one learning rate with torch's defaults (mode 'min', threshold
    1e-4 relative, cooldown 0, min_lr 0, eps 1e-8), on the host"""
    KEYS = ("lr", "best", "num_bad", "cooldown_counter")

    def __init__(self, lr, factor=0.5, patience=10, threshold=1e-4, cooldown=0, min_lr=0.0, eps=1e-8):
        self.lr, self.factor, self.patience, self.threshold, self.cooldown, self.min_lr, self.eps = float(lr), factor, patience, threshold, cooldown, min_lr, eps
        self.best, self.num_bad, self.cooldown_counter = float("inf"), 0, 0

    def step(self, metric):
        metric = float(metric)
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.num_bad = metric, 0
        else:
            self.num_bad += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad = 0
        if self.num_bad > self.patience:
            new = max(self.lr * self.factor, self.min_lr)
            if self.lr - new > self.eps:
                self.lr = new
            self.cooldown_counter, self.num_bad = self.cooldown, 0
        return self.lr

    def state(self):
        return {f"sched_{k}": np.float64(getattr(self, k)) for k in self.KEYS}

    def load(self, st):
        self.lr, self.best = float(st["sched_lr"]), float(st["sched_best"])
        self.num_bad, self.cooldown_counter = int(st["sched_num_bad"]), int(st["sched_cooldown_counter"])


def _train_settings(config):
    """The keys of train_adw, checked (ValueError) before any device work"""
    g = lambda k, d=None: getattr(config, k, d)
    out = {}
    for key, lo, hi, default in (("hidden_size", 1, 1 << 16, None), ("num_layers", 1, 1 << 10, None), ("batch_size", 1, 1 << 16, None),
                                 ("epochs", 1, 1 << 30, None), ("seed", 0, (1 << 63) - 1, 0), ("dim", 1, 16, 1)):
        v = g(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"config.{key} must be an integer in {lo}..{hi}, got {v!r}")
        out[key] = int(v)
    if out["hidden_size"] not in (32, 64, 128, 256):
        raise ValueError(f"config.hidden_size must be 32, 64, 128 or 256, got {out['hidden_size']}")
    for key, positive, default in (("lr", True, None), ("wd", False, 0.0), ("a", True, None), ("max_grad_norm", False, 1.0)):
        v = g(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or np.isnan(v) or (key != "max_grad_norm" and (not np.isfinite(v) or v < 0)) \
                or (positive and v <= 0):
            raise ValueError(f"config.{key} must be a {'finite number > 0' if positive else 'number >= 0'}, got {v!r}")
        out[key] = float(v)
    gamma, t_distr = g("gamma", "brownian"), g("t_distr", "uniform")
    if gamma not in _interp.GAMMAS:
        raise ValueError(f"config.gamma must be one of {_interp.GAMMAS}, got {gamma!r}")
    if t_distr not in ("uniform", "beta"):
        raise ValueError(f"config.t_distr must be 'uniform' or 'beta', got {t_distr!r}")
    for key in ("model_save_path", "model_save_name"):
        if not isinstance(g(key), str) or not g(key):
            raise ValueError(f"config.{key} must be a non-empty string")
    out.update(gamma=gamma, t_distr=t_distr)
    return out


# The draw index of training step k of epoch e is _TRAIN_DRAW0 + e steps + k; validation uses draw = e.  Both draw with the run's seed
# and ids that overlap (rows 0 .. B - 1), so sharing a draw index would hand a training step and a validation batch the same (t, z).
_TRAIN_DRAW0 = 1 << 30


def _split_80_10_10(x, beta, d, rng):
    x = np.ascontiguousarray(C.to_numpy(x, np.float32).reshape((-1,) if d == 1 else (-1, d)))
    beta = np.ascontiguousarray(np.broadcast_to(C.to_numpy(beta, np.float32).reshape(-1), (x.shape[0],)))
    n = x.shape[0]
    perm = rng.permutation(n)
    n_train, n_val = int(0.8 * n), int(0.1 * n)
    tr, va = perm[:n_train], perm[n_train:n_train + n_val]
    return (x[tr], beta[tr]), (x[va], beta[va])


def _train_resume(out_dir, trainer, sched, log):
    """Puts trainer and scheduler back from train_state.npz -> (the epochs done, the log's lists so far)"""
    with np.load(os.path.join(out_dir, "train_state.npz")) as f:
        st = {k: f[k] for k in f.files}
    trainer.load_state_dict(st)
    sched.load(st)
    return int(st["epochs_done"]), {k: list(st["log_" + k]) for k in log}


def _train_checkpoint(out_dir, trainer, sched, log, epochs_done):
    """train_state.npz (optimiser and scheduler state, the epochs done, the log) and log.npz after an epoch"""
    arrs = {k: np.asarray(v) for k, v in log.items()}
    np.savez(os.path.join(out_dir, "train_state.npz"), **trainer.state_dict(), **sched.state(), epochs_done=np.int64(epochs_done),
             **{"log_" + k: v for k, v in arrs.items()})
    np.savez(os.path.join(out_dir, "log.npz"), **arrs)


def train_adw(config, base, target, resume=False):
    """The loop of adw/train.py:18-100 on the GPU.  base / target: (x, beta) array pairs (x [n] or [n, d], beta [n] or one value).
    Both sets are split 80 / 10 / 10 by a seeded permutation.  Per epoch: min(n_train) // batch_size optimiser steps on drop_last
    batches of fresh permutations, in one device loop (Trainer.fit); the validation loss as the mean over the full validation
    batches, without update, at the draws (seed, draw = the epoch, the running row offset) -- the training steps draw from index 2^30
    on, so no step shares its (t, z) with a validation batch; ReduceLROnPlateau(factor 0.5, patience 10)
    on it, then set_lr.  Writes epoch_{k}.npz (the fp64 state dict in the reference's keys), train_state.npz (optimiser and
    scheduler state, the epochs done) and log.npz (train_loss, val_loss, lr, skipped per epoch); resume=True continues from
    train_state.npz.  -> the log as a dict."""
    s = _train_settings(config)
    d, B = s["dim"], s["batch_size"]
    mod = _adw if d == 1 else _adw_nd
    (x0, b0), (v0, vb0) = _split_80_10_10(*base, d, np.random.default_rng([s["seed"], 0]))
    (x1, b1), (v1, vb1) = _split_80_10_10(*target, d, np.random.default_rng([s["seed"], 1]))
    steps, n_val = min(x0.shape[0], x1.shape[0]) // B, min(v0.shape[0], v1.shape[0]) // B
    if steps < 1 or n_val < 1:
        raise ValueError(f"batch_size {B} leaves no full training or validation batch ({x0.shape[0]} / {v0.shape[0]} rows)")
    if s["epochs"] * steps > _TRAIN_DRAW0:
        raise ValueError(f"epochs x steps per epoch = {s['epochs'] * steps} exceeds the {_TRAIN_DRAW0} draw indices of a run")
    out_dir = os.path.join(config.model_save_path, config.model_save_name)
    b = mod.FCNetMultiBeta(d, d, s["hidden_size"], s["num_layers"])
    b.load_state_dict(_adw._syn.make_state_dict(b._spec, seed=s["seed"], dtype=np.float64))
    loss_fn = _losses.StandardVelocityLoss(_interp.LinearInterpolant(s["a"], s["gamma"]), s["t_distr"])
    trainer = _adw.Trainer(b, loss_fn, s["lr"], weight_decay=s["wd"], max_grad_norm=s["max_grad_norm"])
    sched = _Plateau(s["lr"])
    log = dict(train_loss=[], val_loss=[], lr=[], skipped=[])
    first, log = _train_resume(out_dir, trainer, sched, log) if resume else (0, log)
    os.makedirs(out_dir, exist_ok=True)
    for epoch in range(first, s["epochs"]):
        losses, skipped = trainer.fit(x0, x1, b0, b1, B, steps, [s["seed"], 2, epoch], draw=_TRAIN_DRAW0 + epoch * steps, noise_seed=s["seed"])
        val = [trainer.loss(v0[k * B:(k + 1) * B], v1[k * B:(k + 1) * B], vb0[k * B:(k + 1) * B], vb1[k * B:(k + 1) * B], seed=s["seed"],
                            draw=epoch, traj_offset=k * B) for k in range(n_val)]
        log["train_loss"].append(float(np.nanmean(losses)) if skipped < steps else float("nan"))
        log["val_loss"].append(float(np.mean(val)))
        log["skipped"].append(int(skipped))
        log["lr"].append(trainer.lr)
        new_lr = sched.step(log["val_loss"][-1])
        if new_lr != trainer.lr:
            trainer.set_lr(new_lr)
        trainer.sync()
        np.savez(os.path.join(out_dir, f"epoch_{epoch}.npz"), **b.state_dict())
        _train_checkpoint(out_dir, trainer, sched, log, epoch + 1)
    return {k: np.asarray(v) for k, v in log.items()}


def _molecule_train_settings(config, latent):
    """The keys of train_ambient / train_latent, checked (ValueError) before any device work"""
    g = lambda k, d=None: getattr(config, k, d)
    out = {}
    for key, lo, hi, default in (("n_features", 1, 1 << 16, None), ("score_layers", 1, 1 << 10, None), ("batch_size", 1, 1 << 16, None),
                                 ("n_epochs", 1, 1 << 30, None), ("seed", 0, (1 << 63) - 1, 0)):
        v = g(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"config.{key} must be an integer in {lo}..{hi}, got {v!r}")
        out[key] = int(v)
    if out["n_features"] not in (32, 64, 128, 256):
        raise ValueError(f"config.n_features must be 32, 64, 128 or 256, got {out['n_features']}")
    for key, positive, default in (("learning_rate", True, None), ("weight_decay", False, 0.0), ("a", True, 1.0)):
        v = g(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v) or v < 0 or (positive and v <= 0):
            raise ValueError(f"config.{key} must be a {'finite number > 0' if positive else 'finite number >= 0'}, got {v!r}")
        out[key] = float(v)
    gamma, t_distr, align = g("gamma", "brownian"), g("t_distr", "uniform"), g("align", False)
    if gamma not in _interp.GAMMAS:
        raise ValueError(f"config.gamma must be one of {_interp.GAMMAS}, got {gamma!r}")
    if t_distr not in ("uniform", "beta"):
        raise ValueError(f"config.t_distr must be 'uniform' or 'beta', got {t_distr!r}")
    if not isinstance(align, (bool, np.bool_)) or (align and not latent):
        raise ValueError(f"config.align must be a bool (and False for the ambient workflow, which draws no base samples), got {align!r}")
    for key in ("model_save_path", "model_save_name"):
        if not isinstance(g(key), str) or not g(key):
            raise ValueError(f"config.{key} must be a non-empty string")
    radius, cutoff = g("radius_graphs", False), None
    if not isinstance(radius, (bool, np.bool_)) or (radius and latent):
        raise ValueError(f"config.radius_graphs must be a bool (and False for the latent workflow, whose base samples have no graph), got {radius!r}")
    if radius:
        cutoff = g("cutoff")
        if isinstance(cutoff, bool) or not isinstance(cutoff, (int, float, np.integer, np.floating)) or not np.isfinite(cutoff) or cutoff <= 0:
            raise ValueError(f"config.radius_graphs needs config.cutoff, a finite number > 0, got {cutoff!r}")
        cutoff = float(cutoff)
    out.update(gamma=gamma, t_distr=t_distr, align=bool(align), radius_graphs=bool(radius), cutoff=cutoff)
    return out


def _radius_masks(x, cutoff, template, atom_key):
    """masks [n, A] uint32 of a resident set over the template of `template`: bit s of masks[i, d] is set when row i has the edge
    s -> d -- the pairs data.radius_edges gives at `cutoff` (|x_d - x_s| <= cutoff in float64, no self loops), and the template's
    bonded pairs (type > 0), which the reference's bond graph puts into every sample whatever the cutoff."""
    from .thermo._molecule import split_batch
    _, A, src, dst, ety, _ = split_batch(template, atom_key)
    if x.shape[1] != A:
        raise ValueError(f"set0 has {x.shape[1]} atoms per molecule, the template {A}")
    if A > 32:
        raise ValueError(f"per-molecule edge sets need A <= 32 atoms, got {A}")
    bonds = np.zeros(A, np.uint64)
    np.bitwise_or.at(bonds, dst[ety > 0], np.uint64(1) << src[ety > 0].astype(np.uint64))
    bit = np.uint64(1) << np.arange(A, dtype=np.uint64)
    masks = np.empty((x.shape[0], A), np.uint32)
    for lo in range(0, x.shape[0], 4096):
        xs = np.asarray(x[lo:lo + 4096], np.float64)
        near = (np.linalg.norm(xs[:, :, None, :] - xs[:, None, :, :], axis=-1) <= cutoff) & ~np.eye(A, dtype=bool)      # [i, d, s]
        masks[lo:lo + 4096] = ((near * bit).sum(axis=-1, dtype=np.uint64) | bonds).astype(np.uint32)
    return masks


def _molecule_set(s, name):
    """(x [n, A, 3] float32, T [n] float32) of a resident set, checked"""
    if not isinstance(s, (tuple, list)) or len(s) != 2:
        raise ValueError(f"{name} must be (x [n, A, 3], T [n])")
    x = np.ascontiguousarray(C.to_numpy(s[0], np.float32))
    if x.ndim != 3 or x.shape[2] != 3 or x.shape[0] < 1:
        raise ValueError(f"{name}: x must be [n, A, 3], got {x.shape}")
    T = np.ascontiguousarray(np.broadcast_to(C.to_numpy(s[1], np.float32).reshape(-1), (x.shape[0],)))
    return x, T


def _train_molecule(config, set0, set1, template, resume, latent):
    s = _molecule_train_settings(config, latent)
    B = s["batch_size"]
    x1, T1 = _molecule_set(set1, "set1")
    x0, T0 = _molecule_set(set0, "set0") if not latent else (None, None)
    steps = (x1.shape[0] if latent else min(x0.shape[0], x1.shape[0])) // B
    if steps < 1:
        raise ValueError(f"batch_size {B} leaves no full training batch ({x1.shape[0] if latent else min(x0.shape[0], x1.shape[0])} molecules)")
    if s["n_epochs"] * 2 * steps > _TRAIN_DRAW0:
        raise ValueError(f"n_epochs x 2 steps per epoch = {s['n_epochs'] * 2 * steps} exceeds the {_TRAIN_DRAW0} draw indices of a run")
    name = config.model_save_name
    out_dir = os.path.join(config.model_save_path, name)
    temps = getattr(config, "temperatures", _amb.DEFAULT_TEMPS)
    if latent:
        b = _lat.cPaiNN(s["n_features"], s["score_layers"], temp_length=getattr(config, "temp_length", 10), temperatures=temps)
        loss_fn = _losses.OneSidedVelocityLoss(_interp.OneSidedLinearInterpolant(), s["t_distr"])
        trainer = _lat.Trainer(b, loss_fn, s["learning_rate"], weight_decay=s["weight_decay"], max_grad_norm=1.0)
    else:
        b = _amb.cPaiNN(s["n_features"], score_layers=s["score_layers"], temp_length=getattr(config, "temp_length", 10), temperatures=temps)
        loss_fn = _losses.StandardVelocityLoss(_interp.LinearInterpolant(s["a"], s["gamma"]), s["t_distr"])
        trainer = _amb.Trainer(b, loss_fn, s["learning_rate"], weight_decay=s["weight_decay"], max_grad_norm=1.0)
    b.load_state_dict(_adw._syn.make_state_dict(b._spec, seed=s["seed"], dtype=np.float64))
    sched = _Plateau(s["learning_rate"])
    log = dict(train_loss=[], last_train_loss=[], best_loss=[], lr=[], skipped=[])
    first, log = _train_resume(out_dir, trainer, sched, log) if resume else (0, log)
    os.makedirs(out_dir, exist_ok=True)
    if latent:
        sets = (x1, T1 if b.COND_KEYS else None)
        kw = dict(noise="aligned" if s["align"] else "drawn")
    else:
        sets, kw = (x0, T0, x1, T1), {}
        if s["radius_graphs"]:                  # the graphs of set 0, once: a minibatch molecule trains on the graph of its set-0 row
            kw = dict(masks=_radius_masks(x0, s["cutoff"], template, b.ATOM_KEY))
    for epoch in range(first, s["n_epochs"]):
        perm, draw = [s["seed"], 2, epoch], _TRAIN_DRAW0 + epoch * 2 * steps
        losses, skipped = trainer.fit(*sets, B, steps, perm, draw=draw, noise_seed=s["seed"], template_batch=template, track_best=True, **kw)
        last = trainer.evaluate(*sets, B, steps, perm, draw=draw + steps, noise_seed=s["seed"], template_batch=template, **kw)
        best_sd, best_loss, _ = trainer.best_state_dict(reset=True)
        log["train_loss"].append(float(np.nansum(losses)) / steps)          # the reference adds the losses it applied and divides by len(loader)
        log["last_train_loss"].append(float(np.sum(last)) / steps)
        log["best_loss"].append(float(best_loss))
        log["skipped"].append(int(skipped))
        log["lr"].append(trainer.lr)
        new_lr = sched.step(log["train_loss"][-1])
        if new_lr != trainer.lr:
            trainer.set_lr(new_lr)
        trainer.sync()
        np.savez(os.path.join(out_dir, f"{name}_{epoch}_weights.npz"), **b.state_dict())
        np.savez(os.path.join(out_dir, f"{name}_best{epoch}_weights.npz"), **({k: np.asarray(v, np.float32) for k, v in best_sd.items()} if best_sd is not None else b.state_dict()))
        _train_checkpoint(out_dir, trainer, sched, log, epoch + 1)
    return {k: np.asarray(v) for k, v in log.items()}


def train_ambient(config, set0, set1, template, resume=False):
    """The loop of mdqm9/train_ambient.py:99-176 on the GPU.  set0 / set1: (x [n, A, 3], T [n]) arrays of one species, as
    data.load_trajectory gives them per temperature, concatenated by the caller; template: one uniform batch of the species (its graph
    and atom ids build the device trainer).  The sets stay resident on the device.  Per epoch both sets get a fresh seeded permutation
    (the reference makes new loaders every epoch); min(n0, n1) // batch_size optimiser steps run in ONE device call
    (thermo.ambient.Trainer.fit), which also keeps the weights of the step with the smallest loss (epoch_best_model); a second,
    forward-only pass over the same minibatches gives last_train_loss; ReduceLROnPlateau(0.5, 10) acts on the epoch's mean training
    loss, as the reference schedules it.  Stated differences: the reference's loaders keep the ragged last batch, this loop drops it
    (drop_last); permutations, t and z come from numpy's and the library's counter-based streams, not torch's.
    Writes {name}_{epoch}_weights.npz and {name}_best{epoch}_weights.npz (state dicts in the reference's keys, as score_checkpoints
    reads them), train_state.npz (optimiser and scheduler state, the epochs done) and log.npz (train_loss, last_train_loss, best_loss,
    lr, skipped per epoch) under model_save_path/model_save_name; resume=True continues from train_state.npz.  Config: n_features,
    score_layers, batch_size, n_epochs, learning_rate, weight_decay, a, gamma, t_distr, seed, model_save_path, model_save_name
    (align must be False).  Optional radius_graphs (default False; without it the run is what it was): every sample of set 0 trains on
    its own radius graph at config.cutoff (finite, > 0), as the reference's data set builds one per sample and its loss evaluates both
    states on batch0's graph -- masks over the template's edges, built once on the host by the rule of data.radius_edges plus the
    template's bonds, passed to fit / evaluate; the template should then hold every pair a sample can have (the complete graph with
    the species' bond types).  -> the log as a dict."""
    return _train_molecule(config, set0, set1, template, resume, latent=False)


def train_latent(config, set1, template, resume=False):
    """The loop of mdqm9/train_latent.py on the GPU: train_ambient with OneSidedVelocityLoss on one resident set, n1 // batch_size
    steps an epoch.  The base samples x0 of every minibatch (mdqm9_latent.py:84-105: randn_like(x1), centred per molecule, with
    config.align rotated onto x1) are drawn on the device inside the same call, afresh in every epoch; the forward-only pass draws its
    own.  A model with one temperature ignores T.  Files, config keys and differences as train_ambient, plus align."""
    return _train_molecule(config, None, set1, template, resume, latent=True)


MD_KEYS = ("forcefield", "x0", "temperatures", "n_replicas", "dt", "friction", "n_equil", "n_frames", "stride", "seed", "splits",
           "traj_path", "traj_filename")


def _md_settings(config):
    """The keys of generate_md, checked before anything is read or run"""
    from . import data as _data
    missing = [k for k in MD_KEYS if getattr(config, k, None) is None]
    if missing:
        raise ValueError(f"generate_md needs the keys {missing}")
    scale, to_nm = getattr(config, "scale", None), getattr(config, "to_nm", None)
    if (scale is None) == (to_nm is None):
        raise ValueError("generate_md needs exactly one of 'scale' (model units per nm) and 'to_nm' (nm per model unit)")
    v = float(scale if to_nm is None else to_nm)
    if not (np.isfinite(v) and v > 0):
        raise ValueError("'scale' / 'to_nm' must be finite and > 0")
    temps = [int(t) for t in config.temperatures]
    if not temps or len(set(temps)) != len(temps) or any(t not in _data.TEMPERATURES for t in temps):
        raise ValueError(f"'temperatures' must be distinct members of {list(_data.TEMPERATURES)}, got {list(config.temperatures)}")
    n_rep, n_frames, stride, n_equil = int(config.n_replicas), int(config.n_frames), int(config.stride), int(config.n_equil)
    if n_rep < 1 or n_frames < 1 or stride < 1 or n_equil < 0:
        raise ValueError("'n_replicas', 'n_frames' and 'stride' must be >= 1 and 'n_equil' >= 0")
    splits = dict(config.splits)
    frac = np.array([float(f) for f in splits.values()])
    if not len(frac) or (frac <= 0).any() or frac.sum() > 1.0 + 1e-12:
        raise ValueError("'splits' must map split names to positive fractions of the replicas that sum to at most 1")
    counts = np.floor(frac * n_rep + 1e-9).astype(int)          # whole replicas: the splits are independent trajectories
    if (counts < 1).any():
        raise ValueError(f"'splits' {splits} leave a split without a replica at n_replicas = {n_rep}")
    every = getattr(config, "exchange_every", None)             # optional: absent or 0, independent chains
    if every is not None and (isinstance(every, bool) or every != int(every) or int(every) < 0):
        raise ValueError(f"'exchange_every' must be a whole number of steps >= 0 (0: no replica exchange), got {every!r}")
    if every and len(temps) < 2:
        raise ValueError("'exchange_every' needs at least two 'temperatures': a ladder has two rungs or more")
    return (1.0 / v if to_nm is None else v), temps, n_rep, n_frames, stride, n_equil, dict(zip(splits, counts.tolist())), int(every or 0)


def _md_engine(b, A):
    """The engine that runs the dynamics: `b` itself when it is one (a PainnEngine of the species), else the model's engine for the
    fully connected template of A atoms -- the force field needs the species size only"""
    if hasattr(b, "langevin"):
        return b
    from . import synthetic as _syn
    src, dst, et = _syn.fully_connected_template(A)
    return b.engine_for(A, src, dst, et, np.arange(A))


def generate_md(config, b):
    """One batch of Langevin replicas -- n_replicas at every temperature, all advanced together -- written as the training sets of
    train_ambient / train_latent: ``{traj_path}/{split}/{traj_filename}`` float32 [8, n_replicas_in_split * n_frames, A, 3], row
    data.TEMPERATURES.index(T) holding that temperature's frames replica-major (a split takes whole replicas), the rows of
    temperatures that were not simulated NaN; and ``{traj_path}/md_log.npz`` with the per-frame energies, the settings and the seed.
    The frames are centred and in the model's length unit before `scale` (the file load_trajectory(..., scale=False) returns as
    it is).  With the optional key ``exchange_every`` > 0, replica r of every temperature forms one temperature ladder with replica
    exchange after every exchange_every-th step (md.ReplicaExchangeSampler); the files keep their layout and md_log.npz gains
    exchange_every, accept_counts [n_replicas, n_temperatures - 1, 2] (temperatures ascending) and round_trips [n_replicas].
    Returns {split: path}."""
    from . import data as _data
    from . import forcefield as _ff
    from . import md as _md
    to_nm, temps, n_rep, n_frames, stride, n_equil, counts, every = _md_settings(config)
    ff = _ff.ForceField.from_openmm_xml(os.fspath(config.forcefield))
    A = ff.n_atoms
    x0 = np.load(os.fspath(config.x0))
    x0 = x0[None] if x0.ndim == 2 else x0
    if x0.ndim != 3 or x0.shape[1:] != (A, 3) or not np.isfinite(x0).all():
        raise ValueError(f"'x0' must hold finite [{A}, 3] or [n, {A}, 3] geometries, got {x0.shape}")
    B = len(temps) * n_rep                                       # replica r of temperature k is row k * n_replicas + r, its id too
    T = np.repeat(np.asarray(temps, np.float32), n_rep)
    start = x0[np.arange(B) % len(x0)]
    extra = {}
    if not every:
        sampler = _md.LangevinSampler(_md_engine(b, A), ff, to_nm, float(config.dt), float(config.friction), int(config.seed))
        sampler.start(start, T)
        sampler.equilibrate(n_equil)
        frames, epot, ekin = (C.to_numpy(a) for a in sampler.sample(n_frames, stride))
    else:
        # replica exchange: ladder r is made of the rows (T_k, replica r) in ascending temperature.  The library wants the rows
        # ladder-major; every row keeps the id it has above, so a run in which no attempt falls writes the files of the other branch
        order = np.argsort(np.asarray(temps), kind="stable")
        rows = (order[None, :] * n_rep + np.arange(n_rep)[:, None]).reshape(-1)      # ladder-major position -> row
        sampler = _md.ReplicaExchangeSampler(_md_engine(b, A), ff, to_nm, float(config.dt), float(config.friction), int(config.seed), every)
        sampler.start(start[rows], np.asarray(temps, np.float32)[order], n_rep, ids=rows.astype(np.int64))
        sampler.equilibrate(n_equil)
        back = np.argsort(rows)
        frames, epot, ekin = (C.to_numpy(a)[back] for a in sampler.sample(n_frames, stride))
        extra = dict(exchange_every=every, accept_counts=sampler.counts, round_trips=_md.round_trips(sampler.walkers))
    frames = frames.reshape(len(temps), n_rep, n_frames, A, 3)
    paths, first = {}, 0
    for split, n in counts.items():
        out = np.full((len(_data.TEMPERATURES), n * n_frames, A, 3), np.nan, np.float32)
        for k, temp in enumerate(temps):
            out[_data.TEMPERATURES.index(temp)] = frames[k, first:first + n].reshape(n * n_frames, A, 3)
        os.makedirs(os.path.join(config.traj_path, split), exist_ok=True)
        paths[split] = os.path.join(config.traj_path, split, config.traj_filename)
        np.save(paths[split], out)
        first += n
    np.savez(os.path.join(config.traj_path, "md_log.npz"), epot=epot.reshape(len(temps), n_rep, n_frames),
             ekin=ekin.reshape(len(temps), n_rep, n_frames), temperatures=np.asarray(temps), n_replicas=n_rep, dt=float(config.dt),
             friction=float(config.friction), n_equil=n_equil, n_frames=n_frames, stride=stride, seed=int(config.seed), to_nm=to_nm,
             split_names=np.array(list(counts)), split_replicas=np.array(list(counts.values())), **extra)
    return paths
