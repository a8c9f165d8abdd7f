"""ctypes binding of libti_hip.so (the C ABI of include/ti_hip.h).

Fails loudly: there is no CPU fallback.  If the shared library is missing it is NOT silently replaced by anything --
call ``build.build()`` (needs hipcc) or ``__graft_entry__.build()`` first.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# TI_LIB_PATH: explicit path of an alternative build of the library (tools/variant_bench.py builds experiment variants next to
# the product library instead of over it).  Unset in normal use.
SO_PATH = os.environ.get("TI_LIB_PATH") or os.path.join(HERE, "libti_hip.so")

TI_OK, TI_E_ARG, TI_E_HIP, TI_E_NAN, TI_E_ALLOC, TI_E_UNSUPPORTED = 0, -1, -2, -3, -4, -5
MEM_HOST, MEM_DEVICE = 0, 1
SCHEMES = {"euler": 0, "heun": 1, "em": 2, "dopri5": 3, "midpoint": 4, "rk4": 5}
SCHEME_DOPRI5_TRAJ = 6           # dopri5 with per-trajectory step control (engine: scheme="dopri5", step_control="trajectory")
PRECISIONS = {"f32": 0, "f16x2": 1, "f16": 2}
KERNELS = {"painn_edge": 0, "painn_update": 1, "painn_embed": 2, "painn_readout": 3, "adw": 4, "integrate": 5,
           "painn_jvp_edge": 6, "painn_jvp_update": 7, "painn_jvp_readout": 8, "painn_jvp_filter": 9}

# every symbol include/ti_hip.h declares (tests/test_abi.py checks the library exports exactly these)
ABI_SYMBOLS = [
    "ti_rollout_rows", "ti_version", "ti_device_count", "ti_last_error",
    "ti_adw_create", "ti_adw_drift", "ti_adw_drift_div", "ti_adw_rollout", "ti_adw_rollout_dlogp",
    "ti_painn_create", "ti_painn_drift", "ti_painn_rollout", "ti_painn_drift_jvp", "ti_painn_drift_div", "ti_painn_rollout_dlogp",
    "ti_destroy", "ti_set_stream", "ti_wait_stream", "ti_painn_set_template", "ti_painn_template_for", "ti_reserve", "ti_profile_enable", "ti_profile_read",
    "ti_painn_debug_tap", "ti_painn_debug_read", "ti_painn_debug_poison", "ti_selftest",
    "ti_painn_drift_tv", "ti_painn_drift_div_tv", "ti_adw_drift_tv", "ti_rollout_step_counts",
    "ti_painn_drift_div_est", "ti_painn_drift_div_est_tv", "ti_painn_rollout_dlogp_est",
    "ti_adw_create_nd", "ti_painn_set_edge_mask", "ti_painn_set_molecules",
    "ti_obs_cv", "ti_obs_weights", "ti_obs_hist", "ti_obs_set_observer",
    "ti_adw_rollout_fused",
    "ti_obs_bootstrap",
    "ti_painn_debug_phi0_path", "ti_painn_debug_pair_blocks", "ti_painn_debug_pair_seeded", "ti_painn_debug_embed_path", "ti_painn_debug_pair_tails", "ti_painn_debug_update_keep",
    "ti_obs_rff_gram",
    "ti_obs_eigh", "ti_obs_gedmd_spectrum",
    "ti_obs_rff_gram_wide",
    "ti_obs_ff_set", "ti_obs_ff_energy", "ti_obs_ti_logw",
    "ti_obs_zmat", "ti_obs_zmat_xyz", "ti_obs_hist_cols",
    "ti_obs_eigh_wide", "ti_obs_eigh_wide_launch_max", "ti_obs_gedmd_spectrum_wide",
    "ti_painn_vloss", "ti_adw_vloss", "ti_painn_vloss_interp", "ti_adw_vloss_interp",
    "ti_adw_trainer_create", "ti_adw_train_grad", "ti_adw_train_apply", "ti_adw_train_steps", "ti_adw_train_get_state",
    "ti_adw_train_set_state", "ti_adw_train_set_lr",
    "ti_painn_trainer_create", "ti_painn_train_grad", "ti_painn_train_apply", "ti_painn_train_step", "ti_painn_train_get_state",
    "ti_painn_train_set_state", "ti_painn_train_set_lr", "ti_painn_train_workspace_bytes",
    "ti_painn_train_steps", "ti_painn_train_best", "ti_painn_train_noise", "ti_painn_train_set_graphs",
    "ti_obs_ff_forces", "ti_obs_ff_set_masses", "ti_obs_ff_langevin",
    "ti_obs_ff_remd",
    "ti_obs_bg_logw", "ti_obs_bg_ess",
    "ti_obs_tica_moments", "ti_obs_tica_fit", "ti_obs_tica_transform",
]
# CV descriptor kinds (TI_OBS_*)
OBS_KINDS = {"rmsd": 0, "dist": 1, "angle": 2, "torsion": 3, "coord": 4}
# ti_obs_bootstrap: estimators (TI_BOOT_*), filter modes (TI_BOOT_FILTER_*), the fourth counter word of the draws, the most resamples of a call
BOOT_ESTIMATORS = {"ess": 0, "tfep": 1, "mean": 2}
BOOT_FILTERS = {"none": 0, "once": 1, "resample": 2}
BOOT_DOMAIN = 0x424F4F54
BOOT_MAX_RESAMPLES = 1 << 20
# ti_obs_rff_gram: the limits of d and p, and of the feature table (n * P entries, P = p rounded up to 16)
GRAM_MAX_D, GRAM_MAX_P, GRAM_MAX_TABLE = 16, 128, 1 << 27
# ti_obs_rff_gram_wide: the same call with the blocked pass behind it (TI_GRAM_WIDE_MAX_P)
GRAM_WIDE_MAX_P = 1024
# ti_obs_eigh / ti_obs_gedmd_spectrum: the largest matrix order (TI_EIGH_MAX_N), the sweep cap, the most matrices of a call
EIGH_MAX_N, EIGH_MAX_SWEEPS, EIGH_MAX_MATRICES = 64, 64, BOOT_MAX_RESAMPLES + 1
# ti_obs_eigh_wide / ti_obs_gedmd_spectrum_wide: the largest order of the blocked solver (TI_EIGH_WIDE_MAX_N)
EIGH_WIDE_MAX_N = 1024


def eigh_wide_launch_max(n):
    """Matrices of order n one launch of the blocked solver takes (ti_obs_eigh_wide_launch_max: the library's own statement)"""
    return int(lib().ti_obs_eigh_wide_launch_max(int(n)))
# ti_obs_ff_set: the caps of the four tables (TI_FF_MAX_*), R in kJ / (mol K) (TI_FF_GAS_CONSTANT), OpenMM's ONE_4PI_EPS0 in kJ nm / (mol e^2)
FF_MAX_BONDS, FF_MAX_ANGLES, FF_MAX_TORSIONS, FF_MAX_PAIRS = 64, 128, 512, 300
FF_GAS_CONSTANT, FF_COULOMB = 0.00831446261815324, 138.935456
# ti_obs_bg_logw: the most components of a row (TI_BG_MAX_M), log(2 pi) / 2 as the kernel holds it (TI_BG_HALF_LOG_2PI)
BG_MAX_M, BG_HALF_LOG_2PI = 65536, 0.9189385332046727
# ti_obs_ff_langevin: the most steps of one launch when the descriptor leaves it open (TI_MD_DEFAULT_STEPS_PER_LAUNCH)
MD_DEFAULT_STEPS_PER_LAUNCH = 1024
# ti_obs_ff_remd: the most rungs of a ladder (TI_REMD_MAX_RUNGS), the fourth counter word of the exchange draws (TI_REMD_DOMAIN)
REMD_MAX_RUNGS, REMD_DOMAIN = 64, 0x52454D44
# ti_obs_zmat / ti_obs_zmat_xyz: the range of A; ti_obs_hist_cols: the most columns of a call
ZMAT_MIN_ATOMS, ZMAT_MAX_ATOMS, HIST_COLS_MAX = 2, 32, 128
# ti_obs_tica_*: the most lags of a call (TI_TICA_MAX_LAGS), the most value columns (TI_TICA_MAX_K), the scalings of the components
TICA_MAX_LAGS, TICA_MAX_K = 32, 32
TICA_SCALINGS = {"none": 0, "kinetic_map": 1}
# ti_*_vloss: loss kinds (TI_VLOSS_*), gamma kinds (TI_GAMMA_*), centring (TI_CENTER_*), time distributions (TI_TDIST_*), the fourth
# counter word of the time draws, the most bins of a time profile
VLOSS_KINDS = {"standard": 0, "one_sided": 1}
VLOSS_GAMMAS = {"brownian": 0, "sin2": 1, "sig_sum": 2}
VLOSS_CENTERS = {"batch": 0, "molecule": 1, "none": 2}
VLOSS_TDISTS = {"given": 0, "uniform": 1, "beta_half": 2, "beta_2_1": 3}
VLOSS_DOMAIN = 0x564C4F53
VLOSS_MAX_TBINS = 1024
# ti_adw_train_*: the largest minibatch (TI_ADW_TRAIN_MAX_B), the rows of a slice of the weight-gradient contraction
ADW_TRAIN_MAX_B, ADW_TRAIN_ROW_TILE = 1 << 16, 512
# ti_painn_train_*: the rows of a slice of the weight-gradient contraction (TI_PAINN_TRAIN_SLICE), the default workspace budget
PAINN_TRAIN_SLICE, PAINN_TRAIN_DEFAULT_WORKSPACE = 2048, 32 << 30
# ti_painn_train_steps / ti_painn_train_noise: where a minibatch's x0 comes from (TI_NOISE_*)
PAINN_NOISES = {"given": 0, "drawn": 1, "aligned": 2}


class PainnDesc(C.Structure):
    _fields_ = [("variant", C.c_int32), ("n_features", C.c_int32), ("n_layers", C.c_int32), ("n_types", C.c_int32),
                ("n_atoms", C.c_int32), ("n_edges", C.c_int32), ("temp_length", C.c_float), ("time_length", C.c_float),
                ("length_scale", C.c_float), ("temp_mean", C.c_float), ("temp_range", C.c_float), ("precision", C.c_int32)]


class AdwDesc(C.Structure):
    _fields_ = [("hidden_size", C.c_int32), ("num_layers", C.c_int32), ("precision", C.c_int32)]


class RolloutDesc(C.Structure):
    _fields_ = [("scheme", C.c_int32), ("n_step", C.c_int32), ("save_every", C.c_int32), ("mem", C.c_int32),
                ("eps", C.c_float), ("com_free_noise", C.c_int32), ("seed", C.c_uint64), ("traj_offset", C.c_int64),
                ("t_grid", C.POINTER(C.c_float)), ("rtol", C.c_float), ("atol", C.c_float), ("step_offset", C.c_int64)]


class BootDesc(C.Structure):
    _fields_ = [("estimator", C.c_int32), ("filter", C.c_int32), ("k", C.c_double), ("level", C.c_double), ("n_boot", C.c_int64),
                ("first", C.c_int64), ("seed", C.c_uint64)]


class GramDesc(C.Structure):
    _fields_ = [("d", C.c_int32), ("p", C.c_int32), ("n_boot", C.c_int64), ("first", C.c_int64), ("seed", C.c_uint64)]


class GedmdDesc(C.Structure):
    _fields_ = [("d", C.c_int32), ("p", C.c_int32), ("nev", C.c_int32), ("reserved", C.c_int32), ("a", C.c_double), ("tol", C.c_double)]


class TicaDesc(C.Structure):
    _fields_ = [("dim", C.c_int32), ("scaling", C.c_int32), ("reserved", C.c_int32), ("epsilon", C.c_double)]


class FfDesc(C.Structure):
    _fields_ = [("n_bonds", C.c_int32), ("n_angles", C.c_int32), ("n_torsions", C.c_int32), ("n_pairs", C.c_int32), ("coulomb", C.c_double)]


class MdDesc(C.Structure):
    _fields_ = [("dt", C.c_double), ("friction", C.c_double), ("n_steps", C.c_int64), ("stride", C.c_int64), ("step_offset", C.c_int64),
                ("traj_offset", C.c_int64), ("seed", C.c_uint64), ("draw_velocities", C.c_int32), ("steps_per_launch", C.c_int32)]


class RemdDesc(C.Structure):
    _fields_ = [("n_rungs", C.c_int32), ("reserved", C.c_int32), ("exchange_every", C.c_int64)]


class VlossDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("gamma", C.c_int32), ("a", C.c_double), ("center", C.c_int32), ("t_dist", C.c_int32),
                ("seed", C.c_uint64), ("traj_offset", C.c_int64), ("draw", C.c_int32), ("n_tbins", C.c_int32)]


class AdwTrainDesc(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("max_grad_norm", C.c_double)]


class PainnTrainDesc(C.Structure):
    _fields_ = AdwTrainDesc._fields_ + [("max_workspace_bytes", C.c_uint64)]


class PainnStepsDesc(C.Structure):
    _fields_ = [("n_steps", C.c_int64), ("update", C.c_int32), ("noise", C.c_int32), ("track_best", C.c_int32)]


class TiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libti_hip error {code}: {msg}")
        self.code = code


_lib = None


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so (same SONAMEs as /opt/rocm's).  Two HIP
    runtimes in one process cannot both open the GPU ("No HIP GPUs are available" for whichever comes second), so when
    torch is installed libti_hip.so is bound to torch's copy: loading it first (RTLD_GLOBAL) makes the dynamic loader
    resolve libti_hip.so's NEEDED libamdhip64.so.7 to the already-loaded object.  torch itself is not imported."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Load libti_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc, gfx950).  There is no CPU fallback for the sampling path.")
    _preload_torch_hip_runtime()
    L = C.CDLL(SO_PATH)
    fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
    L.ti_rollout_rows.restype = C.c_int64
    L.ti_rollout_rows.argtypes = [C.c_int32, C.c_int32]
    L.ti_last_error.restype = C.c_char_p
    L.ti_painn_create.restype = vp
    L.ti_painn_create.argtypes = [C.POINTER(PainnDesc), fp, C.c_size_t, ip, ip, ip, ip, C.c_int]
    L.ti_painn_drift.argtypes = [vp, vp, C.c_float, vp, C.c_int64, vp, C.c_int]
    L.ti_painn_rollout.argtypes = [vp, C.POINTER(RolloutDesc), vp, vp, C.c_int64, vp, C.POINTER(C.c_int64)]
    L.ti_painn_drift_jvp.argtypes = [vp, vp, vp, C.c_float, vp, C.c_int64, vp, vp, C.c_int]
    L.ti_painn_drift_div.argtypes = [vp, vp, C.c_float, vp, C.c_int64, vp, vp, C.c_int]
    L.ti_painn_rollout_dlogp.argtypes = [vp, C.POINTER(RolloutDesc), vp, vp, C.c_int64, C.c_float, C.c_float, C.c_int, vp, vp, C.POINTER(C.c_int64)]
    L.ti_adw_create.restype = vp
    L.ti_adw_create.argtypes = [C.POINTER(AdwDesc), C.POINTER(C.c_double), C.c_size_t, C.c_int]
    L.ti_adw_create_nd.restype = vp
    L.ti_adw_create_nd.argtypes = [C.POINTER(AdwDesc), C.c_int32, C.POINTER(C.c_double), C.c_size_t, C.c_int]
    L.ti_adw_drift.argtypes = [vp, vp, C.c_float, vp, vp, C.c_int64, vp, C.c_int]
    L.ti_adw_rollout.argtypes = [vp, C.POINTER(RolloutDesc), vp, vp, vp, C.c_int64, vp, C.POINTER(C.c_int64)]
    L.ti_adw_drift_div.argtypes = [vp, vp, C.c_float, vp, vp, C.c_int64, vp, vp, C.c_int]
    L.ti_adw_rollout_dlogp.argtypes = [vp, C.POINTER(RolloutDesc), vp, vp, vp, C.c_int64, vp, vp, C.POINTER(C.c_int64)]
    L.ti_adw_rollout_fused.argtypes = [vp, C.POINTER(RolloutDesc), vp, vp, vp, C.c_int64, vp, vp, C.POINTER(C.c_int64)]
    L.ti_destroy.argtypes = [vp]
    L.ti_destroy.restype = None
    L.ti_set_stream.argtypes = [vp, vp, C.c_int]
    L.ti_wait_stream.argtypes = [vp, vp]
    L.ti_painn_set_template.argtypes = [vp, C.c_int]
    L.ti_painn_template_for.argtypes = [vp, C.c_int64]
    L.ti_reserve.argtypes = [vp, C.c_int64]
    L.ti_profile_enable.argtypes = [vp, C.c_int]
    L.ti_profile_read.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.ti_painn_debug_tap.argtypes = [vp, C.c_int]
    L.ti_painn_debug_read.argtypes = [vp, C.c_int, fp, C.c_size_t]
    L.ti_painn_debug_poison.argtypes = [vp, C.c_int64, C.c_float]
    L.ti_painn_debug_phi0_path.argtypes = [vp, ip]
    L.ti_painn_debug_pair_blocks.argtypes = [vp, ip, ip, ip]
    L.ti_painn_debug_pair_seeded.argtypes = [vp, ip]
    L.ti_painn_debug_embed_path.argtypes = [vp]
    L.ti_painn_debug_update_keep.argtypes = [vp]
    L.ti_painn_debug_pair_tails.argtypes = [vp, ip]
    L.ti_selftest.argtypes = [C.c_int]
    L.ti_painn_drift_tv.argtypes = [vp, vp, vp, vp, C.c_int64, vp, C.c_int]
    L.ti_painn_drift_div_tv.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int]
    L.ti_adw_drift_tv.argtypes = [vp, vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int]
    L.ti_rollout_step_counts.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64]
    L.ti_painn_drift_div_est.argtypes = [vp, vp, C.c_float, vp, C.c_int64, C.c_int32, C.c_uint64, C.c_int64, vp, vp, C.c_int]
    L.ti_painn_drift_div_est_tv.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_uint64, C.c_int64, vp, vp, C.c_int]
    L.ti_painn_rollout_dlogp_est.argtypes = [vp, C.POINTER(RolloutDesc), C.c_int32, C.c_uint64, vp, vp, C.c_int64, C.c_float, C.c_float,
                                             C.c_int, vp, vp, C.POINTER(C.c_int64)]
    L.ti_painn_set_edge_mask.argtypes = [vp, vp, C.c_int64, C.c_int]
    L.ti_painn_set_molecules.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int]
    L.ti_obs_cv.argtypes = [vp, ip, C.c_int32, fp, ip, vp, C.c_int64, vp, C.c_int]
    L.ti_obs_weights.argtypes = [vp, vp, C.c_int64, vp, C.POINTER(C.c_double), C.c_int]
    L.ti_obs_hist.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.c_int]
    L.ti_obs_set_observer.argtypes = [vp, ip, C.c_int32, fp, ip, C.c_int32, vp, C.c_int]
    L.ti_obs_bootstrap.argtypes = [vp, vp, C.c_int64, C.POINTER(BootDesc), vp, C.c_int64, C.POINTER(C.c_double), vp, C.c_int]
    L.ti_obs_rff_gram.argtypes = [vp, vp, C.c_int64, C.c_int64, C.POINTER(C.c_double), vp, C.POINTER(GramDesc), vp, C.c_int64, vp, C.c_int]
    L.ti_obs_rff_gram_wide.argtypes = L.ti_obs_rff_gram.argtypes
    L.ti_obs_eigh.argtypes = [vp, vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_int]
    L.ti_obs_gedmd_spectrum.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_double), C.POINTER(GedmdDesc), vp, vp, vp, C.c_int]
    L.ti_obs_eigh_wide.argtypes = L.ti_obs_eigh.argtypes
    L.ti_obs_eigh_wide_launch_max.restype = C.c_int64
    L.ti_obs_eigh_wide_launch_max.argtypes = [C.c_int32]
    L.ti_obs_gedmd_spectrum_wide.argtypes = L.ti_obs_gedmd_spectrum.argtypes
    dp = C.POINTER(C.c_double)
    L.ti_obs_ff_set.argtypes = [vp, C.POINTER(FfDesc), ip, dp, ip, dp, ip, dp, dp]
    L.ti_obs_ff_energy.argtypes = [vp, vp, C.c_int64, C.c_double, vp, vp, vp, C.c_int]
    L.ti_obs_ti_logw.argtypes = [vp, vp, vp, vp, C.c_int64, vp, C.c_int]
    L.ti_obs_bg_logw.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, C.c_int]
    L.ti_obs_bg_ess.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    L.ti_obs_ff_forces.argtypes = [vp, vp, C.c_int64, C.c_double, vp, vp, vp, C.c_int]
    L.ti_obs_ff_set_masses.argtypes = [vp, dp]
    L.ti_obs_ff_langevin.argtypes = [vp, C.POINTER(MdDesc), vp, vp, vp, vp, C.c_int64, C.c_double, vp, vp, vp, C.c_int]
    L.ti_obs_ff_remd.argtypes = [vp, C.POINTER(MdDesc), C.POINTER(RemdDesc), vp, vp, vp, vp, vp, C.c_int64, C.c_double, vp, vp, vp, vp, vp, vp,
                                 C.c_int]
    L.ti_obs_zmat.argtypes = [vp, ip, ip, vp, C.c_int64, vp, C.c_int]
    L.ti_obs_zmat_xyz.argtypes = [vp, ip, ip, vp, C.c_int64, vp, vp, vp, C.c_int]
    L.ti_obs_hist_cols.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_int]
    i64p = C.POINTER(C.c_int64)
    L.ti_obs_tica_moments.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, i64p, C.c_int64, ip, C.c_int32, vp, vp, vp, C.c_int]
    L.ti_obs_tica_fit.argtypes = [vp, vp, vp, vp, C.c_int32, C.c_int32, C.POINTER(TicaDesc), vp, vp, vp, vp, C.c_int]
    L.ti_obs_tica_transform.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int]
    vd = C.POINTER(VlossDesc)
    L.ti_painn_vloss.argtypes = [vp, vd, vp, vp, vp, vp, vp, C.c_int64, vp, dp, dp, vp, vp, vp, vp, C.c_int]
    L.ti_adw_vloss.argtypes = [vp, vd, vp, vp, vp, vp, vp, vp, C.c_int64, vp, dp, dp, vp, vp, vp, vp, C.c_int]
    L.ti_painn_vloss_interp.argtypes = [vp, vd, vp, vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int]
    L.ti_adw_vloss_interp.argtypes = [vp, vd, vp, vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int]
    L.ti_adw_trainer_create.restype = vp
    L.ti_adw_trainer_create.argtypes = [C.POINTER(AdwDesc), C.c_int32, dp, C.c_size_t, C.POINTER(AdwTrainDesc), C.c_int]
    L.ti_adw_train_grad.argtypes = [vp, vd, vp, vp, vp, vp, vp, vp, C.c_int64, vp, dp, dp, dp, C.c_int]
    L.ti_adw_train_apply.argtypes = [vp, dp, C.POINTER(C.c_int32)]
    L.ti_adw_train_steps.argtypes = [vp, vd, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int64, C.c_int64, dp,
                                     C.POINTER(C.c_int64), C.c_int]
    L.ti_adw_train_get_state.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.ti_adw_train_set_state.argtypes = [vp, dp, dp, dp, C.c_int64]
    L.ti_adw_train_set_lr.argtypes = [vp, C.c_double]
    L.ti_painn_trainer_create.restype = vp
    L.ti_painn_trainer_create.argtypes = [C.POINTER(PainnDesc), dp, C.c_size_t, ip, ip, ip, ip, C.POINTER(PainnTrainDesc), C.c_int]
    L.ti_painn_train_grad.argtypes = [vp, vd, vp, vp, vp, vp, vp, C.c_int64, vp, dp, dp, dp, C.c_int]
    L.ti_painn_train_apply.argtypes = [vp, dp, C.POINTER(C.c_int32)]
    L.ti_painn_train_step.argtypes = [vp, vd, vp, vp, vp, vp, vp, C.c_int64, dp, C.POINTER(C.c_int32), C.c_int]
    L.ti_painn_train_get_state.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.ti_painn_train_set_state.argtypes = [vp, dp, dp, dp, C.c_int64]
    L.ti_painn_train_set_lr.argtypes = [vp, C.c_double]
    L.ti_painn_train_workspace_bytes.restype = C.c_int64
    L.ti_painn_train_workspace_bytes.argtypes = [vp, C.c_int64, C.c_int32]
    L.ti_painn_train_steps.argtypes = [vp, vd, C.POINTER(PainnStepsDesc), vp, C.c_int64, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, dp,
                                       C.POINTER(C.c_int64), C.c_int]
    L.ti_painn_train_best.argtypes = [vp, dp, dp, C.POINTER(C.c_int64), C.c_int]
    L.ti_painn_train_noise.argtypes = [vp, C.c_uint64, C.c_int64, C.c_int32, vp, C.c_int64, C.c_int32, vp, vp, C.c_int]
    L.ti_painn_train_set_graphs.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int]
    _lib = L
    return L


def check(rc):
    if rc != TI_OK:
        raise TiError(rc, lib().ti_last_error().decode())


def last_error() -> str:
    return lib().ti_last_error().decode()


def fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def iptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def as_ptr(buf, *, shape=None, out=False, what="buffer"):
    """(void*, keepalive, is_device, device_index) for a numpy array (host), a torch tensor (cpu or cuda) or a raw int device
    address.  The kernels read and write float32, C-contiguous memory of exactly the documented shape, so anything else is
    refused here instead of being reinterpreted (tensors) or silently copied (a numpy `out` the caller would never see filled)."""
    if buf is None:
        return None, None, False, None
    if isinstance(buf, int):
        return C.c_void_p(buf), None, True, None
    if hasattr(buf, "data_ptr"):                      # torch.Tensor without importing torch
        if str(buf.dtype) != "torch.float32":
            raise TypeError(f"{what} must be float32, got {buf.dtype}")
        if not buf.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        if shape is not None and tuple(buf.shape) != tuple(shape):
            raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(buf.shape)}")
        dev = bool(buf.is_cuda)
        return C.c_void_p(buf.data_ptr()), buf, dev, (buf.device.index if dev else None)
    if out:
        if not isinstance(buf, np.ndarray) or buf.dtype != np.float32 or not buf.flags["C_CONTIGUOUS"] or not buf.flags["WRITEABLE"]:
            raise TypeError(f"{what} must be a writable C-contiguous float32 numpy array (or a torch tensor); it is filled in place")
        a = buf
    else:
        a = np.ascontiguousarray(buf, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(a.shape)}")
    return C.c_void_p(a.ctypes.data), a, False, None
