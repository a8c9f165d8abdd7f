"""Builds libti_hip.so (gfx950) in-tree with hipcc.  `python -m` style entry: build(force=False, jobs=3)."""
from __future__ import annotations

import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libti_hip.so")
SOURCES = ["api_common.hip", "api_painn.hip", "api_adw.hip", "api_vloss.hip", "painn_pack.hip", "painn_host.hip",      # host units (no kernels)
           # host units of the observables (ti_obs_*), one per concern: CVs and the observer, weights, histograms, TI and Boltzmann-
           # generator log-weights, with the reductions the others share; bootstrap and RFF Gram matrices; the eigensolvers and the gEDMD
           # spectra; Z-matrix coordinates; the force field whole (tables, energies, forces, Langevin dynamics, replica exchange)
           "api_obs.hip", "api_obs_resample.hip", "api_obs_eig.hip", "api_obs_zmat.hip", "api_ff.hip",
           "painn_kernels.hip", "painn_edge_nb1.hip", "painn_edge_nb2.hip", "painn_edge_nb4.hip", "painn_edge_nb8.hip",
           "painn_pair_nb1.hip", "painn_pair_nb2.hip", "painn_pair_nb4.hip", "painn_jvp_kernels.hip", "adw_kernels.hip", "ode_kernels.hip",
           # masked twins of the message kernels (per-molecule edge sets), in translation units of their own
           "painn_edge_mask_nb1.hip", "painn_edge_mask_nb2.hip", "painn_edge_mask_nb4.hip", "painn_edge_mask_nb8.hip",
           "painn_pair_mask_nb1.hip", "painn_pair_mask_nb2.hip", "painn_pair_mask_nb4.hip",
           # the pair kernel's builds for the general blocks of a packed template (pair_template.hpp), units of their own like the above
           "painn_pair_gen_nb1.hip", "painn_pair_gen_nb2.hip", "painn_pair_gen_nb4.hip",
           # the seeded twins of the unmasked split-path builds, tile and general (painn_pair_kernel.hpp: SEEDED): units of their own
           # again, so that every older code object stays as it was and the widths compile in parallel
           "painn_pair_seed_nb1.hip", "painn_pair_seed_nb2.hip", "painn_pair_seed_nb4.hip",
           # the merged-tails builds of the seeded general launch (painn_pair_kernel.hpp: TAILS), units of their own once more
           "painn_pair_tails_nb1.hip", "painn_pair_tails_nb2.hip", "painn_pair_tails_nb4.hip",
           # ragged twins of the adaptive-solver kernels (mixed-species batches): a unit of their own, ode_kernels.hip's code stays put
           "ode_ragged_kernels.hip",
           # observables (ti_obs_*): collective variables, importance weights, weighted histograms
           "obs_kernels.hip",
           # a whole fixed-step adw rollout in one launch (ti_adw_rollout_fused): shares the MLP body with adw_kernels.hip (adw_device.hpp)
           "adw_fused_kernels.hip",
           # bootstrap intervals of the weight estimators (ti_obs_bootstrap): a unit of its own, every older code object stays as it was
           "obs_boot_kernels.hip",
           # RFF Gram matrices of resamples on the fp64 matrix cores (ti_obs_rff_gram): a unit of its own again
           "obs_gram_kernels.hip",
           # batched Hermitian Jacobi eigensolver in LDS and the gEDMD algebra around it (ti_obs_eigh, ti_obs_gedmd_spectrum)
           "obs_eig_kernels.hip",
           # the blocked eigensolver from global memory for orders 65..1024 and the wide gEDMD algebra (ti_obs_eigh_wide,
           # ti_obs_gedmd_spectrum_wide): a unit of its own, obs_eig_kernels.hip's code objects stay as they were
           "obs_eig_wide_kernels.hip",
           # force-field energies of a batch and the TI log-weights from them (ti_obs_ff_energy, ti_obs_ti_logw)
           "obs_ff_kernels.hip",
           # Boltzmann-generator log-weights: log N(z; 0, I) of the prior samples and the weight formed from it (ti_obs_bg_logw)
           "obs_bg_kernels.hip",
           # Z-matrix coordinates both ways and the histograms of all columns in one launch (ti_obs_zmat, ti_obs_zmat_xyz, ti_obs_hist_cols)
           "obs_zmat_kernels.hip",
           # velocity loss (ti_painn_vloss, ti_adw_vloss): time draws, interpolant states and centring, per-molecule reduction, batch sums
           "vloss_kernels.hip",
           # adw trainer (ti_adw_train_*): forward / backward / weight-gradient products on the f32 MFMA, fp64 combine, clip + Adam
           "adw_train_kernels.hip", "api_adw_train.hip",
           # molecule trainer (ti_painn_train_*): the forward pass that keeps its intermediates and the reverse pass through cPaiNN
           "painn_train_kernels.hip", "api_painn_train.hip",
           # whole epochs of the molecule trainer (ti_painn_train_steps, ti_painn_train_best, ti_painn_train_noise): the minibatch gather
           # with its conditioning and the best-weights rule; the latent base samples (Philox draw, centring, fp64 Kabsch rotation)
           "painn_steps_kernels.hip", "painn_noise_kernels.hip",
           # layer-0 phi table (class pass, table kernel); the pair kernel's table builds live in painn_pair_nb*.hip
           "painn_phi0_kernels.hip",
           # force-field forces and Langevin dynamics with them (ti_obs_ff_forces, ti_obs_ff_set_masses, ti_obs_ff_langevin): the
           # kernels, which share the per-term gradients of ff_device.hpp; obs_ff_kernels.hip's code object stays as it was
           "obs_ff_md_kernels.hip",
           # replica exchange between the Langevin launches (ti_obs_ff_remd): the attempt kernel, a unit of its own; its entry point
           # lives in api_ff.hip next to ti_obs_ff_langevin's, the table staging both kernel units share in ff_stage.hpp
           "obs_ff_remd_kernels.hip",
           # the update kernel's builds that keep v_eff in registers (painn_update_kernel_body.inc: KEEP): a unit of its own, the code
           # objects of painn_kernels.hip stay as they were
           "painn_update_keep.hip",
           # TICA (ti_obs_tica_moments, ti_obs_tica_fit, ti_obs_tica_transform): the lagged moments on the fp64 matrix cores, the
           # algebra around the two solves of obs_eig_kernels.hip and the projection; its entry points, a host unit of their own
           "obs_tica_kernels.hip", "api_obs_tica.hip",
           # the molecule trainer on per-molecule graphs (ti_painn_train_set_graphs): masked / ragged twins of the trainer's kernels
           # that read the graph or the loss rows, a unit of their own.  A twin and its parent are one body (vloss_state_body.inc,
           # painn_train_graph_body.inc) included by both units, so the code objects of vloss_kernels.hip and painn_train_kernels.hip
           # stay as they were by construction: there every predicate is `false`, nothing or the plain expression
           "painn_train_graph_kernels.hip"]
HEADERS = ["ti_handle.hpp", "rollout.hpp", "mfma_chain.hpp", "dispatch.hpp", "ti_internal.hpp", "adw_train.hpp", "painn_train.hpp", "painn_train_graph.hpp", "painn_steps.hpp", "train_optim.hpp", "ode_device.hpp", "adw_device.hpp", "boot_draw.hpp", "vloss_normal.hpp", "vloss_device.hpp", "ff_device.hpp", "ff_stage.hpp", "painn_edge_kernel.hpp", "painn_pair_kernel.hpp", "pair_template.hpp", "message_stream.hpp", "painn_update_kernel.hpp",
           "painn_edge_kernel_body.inc", "painn_pair_kernel_body.inc", "painn_update_kernel_body.inc", "painn_embed_kernel_body.inc", "painn_jvp_edge_body.inc", "painn_jvp_filter_body.inc", "vloss_state_body.inc", "painn_train_graph_body.inc", os.path.join("..", "..", "include", "ti_hip.h")]
# -packed-fp32-ops off: v_pk_{fma,mul,add}_f32 do NOT run next to another wave's matrix instructions on gfx950 (a wave of them and a
# wave of 16x16x32 fp16 MFMAs on one SIMD take the SUM of their times; scalar v_fma_f32, conversions and transcendentals overlap:
# tools/micro/coexec_classes.hip, profiles/r03i_microbench_coexec.txt), and register pairs cost the message kernels registers (pair
# kernel: 19 -> 4 spilled).  Measured, same box: pair message kernel -2.0 %, directed -0.6 %, divergence workload +1.2 %
# (profiles/r03i_nopk_timing.txt); results move in the last bit (fma contraction), parity unchanged.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
# Per-source flags.  painn_edge_nb8.hip (F = 256, one wave per SIMD): hipcc (ROCm 7.2) spills 28 SGPRs of the one-accumulator message
# kernel into lanes of a VGPR, and that build faults on the device in its first launch (HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION,
# profiles/r02h_f256_one_chain_fault.txt); the same source with the lane spills switched off allocates them to registers (no scratch) and
# passes every stage at 1.6e-6 (profiles/r03e_f256_one_chain_no_lane_spill.txt).  DESIGN.md 3.4.
EXTRA_FLAGS = {"painn_edge_nb8.hip": ["-mllvm", "-amdgpu-spill-sgpr-to-vgpr=0"], "painn_edge_mask_nb8.hip": ["-mllvm", "-amdgpu-spill-sgpr-to-vgpr=0"]}


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found (need ROCm to build libti_hip.so)")
    return exe


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, jobs: int = 8, verbose: bool = False) -> str:
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS]
    if not force and not _stale(SO, deps):
        return SO
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    cc = hipcc()

    def compile_one(src):
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or _stale(obj, [os.path.join(CSRC, src)] + [os.path.join(CSRC, h) for h in HEADERS]):
            cmd = [cc, *FLAGS, *EXTRA_FLAGS.get(src, []), "-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    subprocess.check_call([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO, *objs])
    return SO


if __name__ == "__main__":
    print(build(verbose=True))
