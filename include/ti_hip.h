/*
 * ti_hip.h -- C ABI of libti_hip.so, the MI355X (gfx950) sampler hot path for thermodynamic-interpolation.
 *
 * The reference (olsson-group/thermodynamic-interpolation) is pure Python and has no FFI seam; the seam this
 * library sits under is the reference's Python API for the sampling path.  Each entry point names the
 * reference interface it replaces (paths relative to the reference checkout):
 *
 *   ti_adw_create / ti_adw_drift      FCNetMultiBeta.__init__/forward      adw/thermo/models/simple.py:11-41
 *                                     + ODEWrapper.forward                 adw/thermo/models/ode_wrapper.py:30-52
 *   ti_adw_rollout                    StandardIntegrator.rollout           adw/thermo/integrators.py:33-68
 *   ti_adw_create_nd                  FCNetMultiBeta(d, d, H, L), 1 <= d <= 16  adw/thermo/models/simple.py:11-41
 *   ti_painn_create / ti_painn_drift  cPaiNN.__init__/forward              mdqm9/thermo/ambient/models/cpainn.py:23-115
 *                                                                          mdqm9/thermo/latent/models/cpainn.py:23-108
 *                                     + ODEWrapper.forward/reset_batch     mdqm9/thermo/{ambient,latent}/models/ode_wrapper.py
 *   ti_painn_rollout                  MoleculeIntegrator.rollout           mdqm9/thermo/ambient/integrators.py:28-68
 *                                                                          mdqm9/thermo/latent/integrators.py:41-89
 *   ti_painn_drift_div / _jvp         ODEWrapper.compute_divergence        mdqm9/thermo/{ambient,latent}/models/ode_wrapper.py:59-91
 *   ti_painn_rollout_dlogp            MoleculeIntegrator.rollout(return_dlogp=True), ODEWrapper.forward (b, -div)
 *   ti_painn_drift_tv / _div_tv       cPaiNN.forward / ODEWrapper.compute_divergence with one batch.t per molecule
 *                                     (mdqm9/thermo/ambient/losses.py:45-70 feeds such batches)
 *   ti_adw_drift_tv                   FCNetMultiBeta.forward with per-row ts                adw/thermo/models/simple.py:38-41
 *   ti_painn_drift_div_est / _est_tv  no reference counterpart: Hutchinson's estimate of the divergence ODEWrapper.compute_divergence
 *   ti_painn_rollout_dlogp_est        computes exactly (the FFJORD estimator; the reference ships the exact one only)
 *   ti_painn_vloss / ti_adw_vloss     StandardVelocityLoss / OneSidedVelocityLoss.forward   mdqm9/thermo/{ambient,latent}/losses.py, adw/thermo/losses.py
 *   + ti_*_vloss_interp               with LinearInterpolant / OneSidedLinearInterpolant    .../interpolants.py (forward evaluation only)
 *   ti_adw_trainer_create, ti_adw_train_*  the training loop's step: backward, clip_grad_norm_, Adam  adw/train.py:18-100
 *   TI_SCHEME_DOPRI5_TRAJ             the reference's dopri5 integration (integrators.py, odeint per mini-batch) evaluated for every
 *   + ti_rollout_step_counts          trajectory as if it were alone in its batch (a batch size of 1)
 *
 * Conventions
 *   - Plain pointers and sizes only; no exceptions cross the ABI.  Every int-returning call returns TI_OK (0) or a
 *     negative TI_E* code; ti_last_error() returns a thread-local message for the last failure on this thread.
 *   - The caller owns every buffer it passes.  Weights/graph templates are copied at create(); the handle owns all
 *     device memory and is freed only by ti_destroy().
 *   - Buffers marked [host|device] are interpreted according to ti_rollout_desc.mem / the `mem` argument:
 *     TI_MEM_HOST = ordinary host memory (the library stages through HBM), TI_MEM_DEVICE = pointers into HBM of
 *     the handle's device (e.g. torch.Tensor.data_ptr()); device work is enqueued on the handle's stream and the
 *     call returns after that stream has been synchronised.
 *   - There is no CPU fallback: if no gfx950 device is usable, create() fails with TI_E_HIP.
 *   - Environment (read per call): TI_TEMPLATE=throughput|latency|pair pins the edge-row layout that is otherwise chosen from
 *     the batch size (results agree to fp32 round-off; bit-identical within one layout); TI_JVP_WS_GB = HBM budget in GB for the
 *     tangent state of the divergence (default 48).
 *
 * Weight layout ("canonical flat layout", fp32 unless noted; every tensor row-major in torch's [out, in] order)
 *   MLP(f_in, f_h, f_out) := W0[f_h,f_in] b0[f_h] g0[f_h] be0[f_h]  W1[f_h,f_h] b1[f_h] g1[f_h] be1[f_h]  W2[f_out,f_h] b2[f_out]
 *                            (Linear, LayerNorm(gamma g, beta be, eps 1e-5), SiLU, Linear, LayerNorm, SiLU, Linear;
 *                             mdqm9/thermo/ambient/models/embedding.py:27-35)
 *   painn :  edge_emb[4,F]  atom_emb[n_types,F]  MLP(nE*F, F, F)
 *            L x { phi = MLP(2F,F,5F)  w = MLP(F,F,5F)  U[F,F]  V[F,F]  upd = MLP(2F,F,3F) }
 *            readout MLP(F,F,2)  Vr[1,F]
 *            nE = 4 (ambient: atom|T0|T1|t), 3 (latent multi-T: atom|T|t), 2 (latent single-T: atom|t)
 *   adw   :  beta_embed: W[H,3] b[H] W[H,H] b[H] W[1,H] b[1] ;  net: W[H,3] b[H] (W[H,H] b[H]) x (num_layers-1) W[1,H] b[1]
 *            dimension d (ti_adw_create_nd):  net: W[H,d+2] b[H] (W[H,H] b[H]) x (num_layers-1) W[d,H] b[d]  (inputs [x, t, embed])
 *            passed as fp64 (the reference trains/saves in float64, adw/train.py:29); the device computes in fp32.
 */
#ifndef TI_HIP_H
#define TI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TI_ABI_VERSION 5

enum { TI_OK = 0, TI_E_ARG = -1, TI_E_HIP = -2, TI_E_NAN = -3, TI_E_ALLOC = -4, TI_E_UNSUPPORTED = -5 };
enum { TI_MEM_HOST = 0, TI_MEM_DEVICE = 1 };
enum { TI_VARIANT_AMBIENT = 0, TI_VARIANT_LATENT_MULTI = 1, TI_VARIANT_LATENT_SINGLE = 2 };
enum { TI_PREC_F32 = 0, TI_PREC_F16X2 = 1, TI_PREC_F16 = 2 };
/* Fixed-step schemes on a caller-supplied grid t[0..n_step-1] (the reference passes torch.linspace(start,end,n_step),
 * integrators.py:43; reversed grid for reverse_ode).  Build-defined (SURVEY.md F3 / §8a row I-new):
 *   EULER: x_{k+1} = x_k + dt_k b(x_k,t_k)                  (== torchdiffeq method='euler' on that grid)
 *   HEUN : xp = x_k + dt_k b(x_k,t_k); x_{k+1} = x_k + dt_k/2 (b(x_k,t_k) + b(xp,t_{k+1}))
 *   EM   : x_{k+1} = x_k + dt_k b(x_k,t_k) + sqrt(2 eps |dt_k|) xi,  xi ~ N(0,1) from Philox4x32-10 keyed by
 *          (seed, global trajectory id, step, component); eps = 0 reproduces EULER bit-for-bit. */
enum { TI_SCHEME_EULER = 0, TI_SCHEME_HEUN = 1, TI_SCHEME_EM = 2,
       /* torchdiffeq 0.2.5 solvers (the reference's integrator library, ti_env.yml:14; third-party, restated from its published
        * algorithm -- parity unpinned):
        *   DOPRI5   : adaptive Dormand-Prince 5(4) with FSAL, step control err = rms((y1_err)/(atol + rtol max(|y0|,|y1|))) <= 1
        *              (two-state runs: max of the per-state rms), factor = min(10, max(0.9 err^(-1/5), 0.2 | 1)), initial step
        *              by Hairer's rule, quartic dense output evaluated at the grid times (the grid only selects output times);
        *   MIDPOINT : fixed grid, y += dt f(t + dt/2, y + dt/2 f(t, y));
        *   RK4      : fixed grid, the 3/8-rule (torchdiffeq's `rk4`). */
       TI_SCHEME_DOPRI5 = 3, TI_SCHEME_MIDPOINT = 4, TI_SCHEME_RK4 = 5,
       /*   DOPRI5_TRAJ: DOPRI5 with per-trajectory step control -- every trajectory (a molecule's 3A coordinates, an adw particle; plus
        *              its dlogp entry) has its own initial step, error ratio (its own mixed norm), accept / reject decisions, step sizes
        *              and dense output, i.e. exactly what DOPRI5 gives for that trajectory in a batch of one; the result does not depend
        *              on the batch, its order or the sharding.  The batch runs until its last trajectory has reached the end of the
        *              grid (finished ones are evaluated along, never written); *n_fevals counts batched evaluations (2 + 6 x the most
        *              attempts any trajectory took); ti_rollout_step_counts returns the per-trajectory counts.  Same rtol / atol. */
       TI_SCHEME_DOPRI5_TRAJ = 6 };

typedef struct ti_handle ti_handle;

typedef struct ti_painn_desc {
    int32_t variant;        /* TI_VARIANT_* */
    int32_t n_features;     /* F: multiple of 32, <= 256 */
    int32_t n_layers;       /* L = score_layers */
    int32_t n_types;        /* rows of the atom embedding (reference: 25) */
    int32_t n_atoms;        /* A atoms per molecule (every molecule of a batch shares one species) */
    int32_t n_edges;        /* E_m directed edges per molecule */
    float   temp_length;    /* PositionalEncoder max_length for temperatures */
    float   time_length;    /* ... for t (reference: 10) */
    float   length_scale;   /* ... for edge distances (reference: 10) */
    float   temp_mean;      /* mean(temperatures)            (embedding.py:209) */
    float   temp_range;     /* max(temperatures) - min(...)  (embedding.py:210) */
    int32_t precision;      /* TI_PREC_F32: f32 MFMA (default); TI_PREC_F16X2: the matrix products on the fp16 matrix rate with
                               every fp32 operand split into two fp16 halves (products hi*hi, hi*lo, lo*hi; fp32 accumulation;
                               ~24 significand bits; un-normalised operand rows are scaled by a power of two first, so any fp32
                               magnitude works; weights must be < 65504).  Two operand formats are in use:
                                 (a) "two accumulators": x = hi + 2^-11 lo with lo = fp16(2^11 (x - hi)); the cross terms have an
                                     accumulator of their own that is folded back with 2^-11.  Used by the update / embed / readout /
                                     tangent kernels at every width and by the message kernels at F = 256;
                                 (b) "one accumulator" (message kernels, F <= 128): each weight matrix is scaled on the host by a
                                     power of two S to the top of the fp16 range, lo = fp16(S w - hi) and lo = fp16(x - hi) are NOT
                                     scaled, and all three products add into one register set (S cancels in the LayerNorm behind
                                     a hidden layer and is divided out of the output products).  It relies on
                                     v_mfma_f32_16x16x32_f16 taking fp16-subnormal inputs at face value, which ti_selftest checks;
                               TI_PREC_F16: fp16 STORAGE mode (BASELINE.json configs[4]): the state tensors s, v, P, e live in HBM
                               as fp16 and every matrix product is one fp16 MFMA with fp32 accumulation; LayerNorm, SiLU,
                               sin/cos, per-atom sums and the integrator state x stay fp32.  A separately labelled precision:
                               drift rel-L2 ~1e-3 against the reference (not the 1e-5 of the other two); values must stay
                               inside the fp16 range; no divergence / dlogp / debug taps in this mode (TI_E_UNSUPPORTED) */
} ti_painn_desc;

typedef struct ti_adw_desc {
    int32_t hidden_size;    /* H: multiple of 32, <= 256 */
    int32_t num_layers;     /* number of hidden layers of `net` (reference: 5) */
    int32_t precision;      /* TI_PREC_F32 | TI_PREC_F16X2 (as ti_painn_desc.precision) */
} ti_adw_desc;

typedef struct ti_rollout_desc {
    int32_t scheme;         /* TI_SCHEME_* */
    int32_t n_step;         /* number of grid points; n_step-1 steps are taken */
    int32_t save_every;     /* k>=1: rows 0,k,2k,... of the path plus the final state are written; 0: final state only */
    int32_t mem;            /* TI_MEM_* for x0 / cond / out_path */
    float   eps;            /* EM noise scale (>= 0) */
    int32_t com_free_noise; /* EM, molecules: remove the per-molecule centre of mass of xi */
    uint64_t seed;          /* EM Philox key */
    int64_t traj_offset;    /* global index of trajectory 0 of this call (multi-GPU shards keep RNG independent of the split) */
    const float* t_grid;    /* [n_step] host memory */
    float   rtol, atol;     /* DOPRI5 tolerances (> 0); ignored by the fixed-grid schemes */
    int64_t step_offset;    /* EM: index of this call's first step in the noise counter (step k of the call draws with counter
                               step_offset + k), so that a trajectory continued by a second call does not reuse the first call's
                               noise; 0 for a rollout that starts at the beginning */
} ti_rollout_desc;

/* number of path rows ti_*_rollout writes for (n_step, save_every) */
int64_t ti_rollout_rows(int32_t n_step, int32_t save_every);

int ti_version(void);
int ti_device_count(void);
const char* ti_last_error(void);

/* ---- adw: asymmetric double well (1-D) and FCNetMultiBeta toy systems in d dimensions ----------------------------- */
ti_handle* ti_adw_create(const ti_adw_desc* desc, const double* weights, size_t n_weights, int device);
/* FCNetMultiBeta(d, d, H, L): the drift of a d-dimensional toy system, 1 <= d <= 16 (TI_E_UNSUPPORTED otherwise); the weight
 * count is that of the layout above (TI_E_ARG otherwise).  Both are checked before any device call.  ti_adw_create is dim = 1.
 * With a d-dimensional handle the adw calls below take  x, out, x0: [B, d] row-major;  out_path: [rows, B, d];
 * beta0, beta1, t, out_div: [B];  out_dlogp: [rows, B].  out_div[i] = sum_k d b_ik / d x_ik, the exact divergence (forward mode,
 * d directions).  EM noise: coordinate k of a particle is component k of the TI_SCHEME_EM draw.  DOPRI5_TRAJ: a particle's
 * error ratio is the rms over its d entries, maxed with its dlogp entry's.
 * TI_PREC_F16X2 (both create calls): every weight must be finite and below 65504 in magnitude (TI_E_UNSUPPORTED names the first
 * that is not; checked before any device call).  The mode holds the f32 path's parity while every hidden activation (SiLU output)
 * stays below 65504 in magnitude: the split operands are unscaled, so beyond that the affected rows are non-finite and rollouts
 * report TI_E_NAN.  Tangent rows below ~1e-6 lose relative, not absolute, accuracy in out_div.  TI_PREC_F32 has neither limit. */
ti_handle* ti_adw_create_nd(const ti_adw_desc* desc, int32_t dim, const double* weights, size_t n_weights, int device);
/* b[i] = net([x_i, t, beta_embed([beta0_i, beta1_i, t])]);  x,beta0,beta1,out: [B] fp32 [host|device] ([B, d] x / out: see above) */
int ti_adw_drift(ti_handle* h, const float* x, float t, const float* beta0, const float* beta1, int64_t B, float* out, int mem);
/* also out_div[i] = d b_i / d x_i, the exact divergence of the 1-D drift by forward-mode differentiation of `net`
 * (ODEWrapper.compute_divergence, adw/thermo/models/ode_wrapper.py:55-67, without its 1e-2 factor) */
int ti_adw_drift_div(ti_handle* h, const float* x, float t, const float* beta0, const float* beta1, int64_t B, float* out,
                     float* out_div, int mem);
/* ti_adw_drift / ti_adw_drift_div with one time per row: t [B] fp32 [host|device] (FCNetMultiBeta.forward with per-row ts,
 * adw/thermo/models/simple.py:38-41); out_div may be NULL.  A uniform t equals ti_adw_drift(_div) bit for bit. */
int ti_adw_drift_tv(ti_handle* h, const float* x, const float* t, const float* beta0, const float* beta1, int64_t B, float* out,
                    float* out_div, int mem);
/* out_path: [rows, B] fp32 with rows = ti_rollout_rows(...) */
int ti_adw_rollout(ti_handle* h, const ti_rollout_desc* desc, const float* x0, const float* beta0, const float* beta1,
                   int64_t B, float* out_path, int64_t* n_fevals);
/* StandardIntegrator(return_dlogp=True) (adw/thermo/integrators.py:38-68): integrates the second state
 * d(dlogp)/dt = -div * 1e-2 with the same scheme (any but EM with eps > 0) and writes out_dlogp [rows, B] = dlogp * 1e2 */
int ti_adw_rollout_dlogp(ti_handle* h, const ti_rollout_desc* desc, const float* x0, const float* beta0, const float* beta1,
                         int64_t B, float* out_path, float* out_dlogp, int64_t* n_fevals);
/* ti_adw_rollout / ti_adw_rollout_dlogp (out_dlogp != NULL) of a 1-D handle with the whole step loop inside ONE kernel launch: a wave
 * keeps its 16 particles in registers for all n_step - 1 steps, evaluates `net` (and its d/dx tangent), applies the state update,
 * draws the EM noise and writes only the rows save_every asks for; the beta embedding of every grid point comes from one launch of
 * the embedding kernel ahead of it (a table of n_step x distinct (beta0, beta1) pairs, at most 2^24 rows: TI_E_UNSUPPORTED beyond).
 * Same descriptor, shapes, *n_fevals (n_step - 1, twice that for HEUN) and TI_E_NAN check as the unfused calls, and the same result
 * BIT FOR BIT: both run one MLP source, the per-step scalars (dt, dt / 2, -dt 1e-2, sqrt(2 eps |dt|)) are computed on the host by
 * the unfused loop's fp32 expressions, and the updates are the fused multiply-adds its update kernels compile to.
 * Opt-in: no other call changes what it launches.
 * TI_E_ARG: a NULL or non-adw handle, NULL buffers with B > 0 (out_dlogp may be NULL).  TI_E_UNSUPPORTED, before any device work: a
 * handle with dim > 1 (use ti_adw_rollout), a scheme other than EULER / HEUN / EM, EM with eps > 0 together with out_dlogp, an
 * attached observer (the rows are written inside the kernel).  B = 0: TI_OK, *n_fevals = 0.  Profile slot: TI_KERNEL_ADW (2 launches). */
int ti_adw_rollout_fused(ti_handle* h, const ti_rollout_desc* desc, const float* x0, const float* beta0, const float* beta1,
                         int64_t B, float* out_path, float* out_dlogp /* may be NULL */, int64_t* n_fevals);

/* ---- mdqm9: cPaiNN drift over homogeneous molecule batches ------------------------------------------------------ */
/* edge_src/edge_dst: [E_m] local atom indices of ONE molecule in the reference's (src,dst)-sorted order
 * (edge_index[0]=src, edge_index[1]=dst: messages flow src -> dst, cpainn.py:273-304); edge_type: [E_m] in 0..3;
 * atom_ids: [A] rows of the atom embedding (reference: arange(A), mdqm9_ambient.py:219-220). */
ti_handle* ti_painn_create(const ti_painn_desc* desc, const float* weights, size_t n_weights,
                           const int32_t* edge_src, const int32_t* edge_dst, const int32_t* edge_type,
                           const int32_t* atom_ids, int device);
/* x: [B,A,3]; cond: [B,A,n_cond] per-node conditioning (ambient: T0,T1; latent multi-T: T; single-T: NULL); out: [B,A,3] */
int ti_painn_drift(ti_handle* h, const float* x, float t, const float* cond, int64_t B, float* out, int mem);
/* ti_painn_drift with one time per molecule: t [B] fp32 [host|device] -- the reference's per-node batch.t, constant within a molecule
 * (cPaiNN.forward, cpainn.py:23-115; the training losses feed one t per molecule, mdqm9/thermo/ambient/losses.py:45-70).
 * A uniform t equals ti_painn_drift bit for bit, and row b equals ti_painn_drift at t[b] (same B, same layout). */
int ti_painn_drift_tv(ti_handle* h, const float* x, const float* t, const float* cond, int64_t B, float* out, int mem);
/* out_path: [rows, B, A, 3]; *n_fevals = drift evaluations taken (DOPRI5: 2 + 6 per attempted step) */
int ti_painn_rollout(ti_handle* h, const ti_rollout_desc* desc, const float* x0, const float* cond, int64_t B,
                     float* out_path, int64_t* n_fevals);

/* Forward-mode derivative of the drift along xdot [B,A,3]: out = b(x), out_tan = (d b / d x) xdot.  The building block
 * of the divergence below; also what the parity tests tap stage by stage. */
int ti_painn_drift_jvp(ti_handle* h, const float* x, const float* xdot, float t, const float* cond, int64_t B, float* out,
                       float* out_tan, int mem);
/* Exact divergence out_div[b] = sum_{a,c} d b[b,a,c] / d x[b,a,c] by 3A unit-seed forward-mode passes per molecule --
 * what ODEWrapper.compute_divergence obtains with 3A reverse-mode passes (mdqm9/thermo/ambient/models/ode_wrapper.py:59-91,
 * latent/models/ode_wrapper.py:57-86), WITHOUT the ambient wrapper's 1e-2 factor.  Tangent state is processed in chunks of
 * molecules sized to TI_JVP_WS_GB gigabytes of HBM (environment, default 48). */
int ti_painn_drift_div(ti_handle* h, const float* x, float t, const float* cond, int64_t B, float* out, float* out_div, int mem);
/* ti_painn_drift_div with one time per molecule, t [B] (ODEWrapper.compute_divergence at a per-molecule batch.t) */
int ti_painn_drift_div_tv(ti_handle* h, const float* x, const float* t, const float* cond, int64_t B, float* out, float* out_div, int mem);
/* MoleculeIntegrator.rollout(return_dlogp=True) (ambient/integrators.py:36-68, latent/integrators.py:57-89) on the fixed
 * grid of `desc` (EULER, HEUN, MIDPOINT, RK4 or the adaptive DOPRI5; EM is refused): second state d(dlogp)/dt = -div_scale * div, or with reverse_ode the pair
 * (-b, +div_scale * div) (ode_wrapper.py:49; the caller passes the descending grid linspace(end, start)).
 * out_dlogp [rows, B] = state * out_scale.  Reference values: ambient div_scale 1e-2, out_scale 1e2; latent 1, 1. */
int ti_painn_rollout_dlogp(ti_handle* h, const ti_rollout_desc* desc, const float* x0, const float* cond, int64_t B,
                           float div_scale, float out_scale, int reverse_ode, float* out_path, float* out_dlogp, int64_t* n_fevals);

/* Hutchinson's trace estimator, an unbiased but noisy replacement for the exact divergence above: k = n_probes Rademacher
 * probes per molecule instead of 3A unit seeds (k tangent directions per evaluation instead of 3A).  Definition:
 *   probe p in [0, k) of trajectory b (global id traj_offset + b), atom a, component c:
 *     eps[b,p,a,c] = +1 if N(probe_seed, traj_offset + b, p, 3a + c) >= 0 else -1      (exactly 0 -> +1)
 *   with N the Philox normal of TI_SCHEME_EM, the probe index in its step slot and the component index 3a + c that the molecule
 *   noise uses (oracle.normal(probe_seed, traj, p, 3a + c) regenerates every probe on the host);
 *   out_div[b] = (1/k) sum_p sum_{a,c} eps[b,p,a,c] (J_b eps[b,p])[a,c],  J_b = d b(x_b) / d x_b  -- WITHOUT the 1e-2 factor, like
 *   ti_painn_drift_div.  E[out_div] = tr J_b; the variance is (2/k) sum_{i != j} ((J_ij + J_ji) / 2)^2.
 * The probes depend on (probe_seed, global trajectory id) only and are FIXED for the whole call (the FFJORD convention): a rollout
 * draws them once, from desc->traj_offset, and uses them at every evaluation, so the dlogp state follows a deterministic ODE -- every
 * scheme (the fixed-grid ones as well as DOPRI5 / DOPRI5_TRAJ, whose error control applies unchanged) integrates it as it integrates
 * the exact one; a chained call with the same ids reuses the same probes, and the result does not depend on the batch composition,
 * order or sharding once the template is pinned.  Redrawing per step is not offered.  n_probes < 1: TI_E_ARG; TI_PREC_F16:
 * TI_E_UNSUPPORTED.  The sum over probes and components runs in a fixed order (deterministic). */
int ti_painn_drift_div_est(ti_handle* h, const float* x, float t, const float* cond, int64_t B, int32_t n_probes, uint64_t probe_seed,
                           int64_t traj_offset, float* out, float* out_div, int mem);
/* ti_painn_drift_div_est with one time per molecule, t [B] [host|device] */
int ti_painn_drift_div_est_tv(ti_handle* h, const float* x, const float* t, const float* cond, int64_t B, int32_t n_probes,
                              uint64_t probe_seed, int64_t traj_offset, float* out, float* out_div, int mem);
/* ti_painn_rollout_dlogp with the estimate in place of the exact divergence (same schemes, EM refused, same scales and reverse_ode);
 * the probes of trajectory b are those of global id desc->traj_offset + b. */
int ti_painn_rollout_dlogp_est(ti_handle* h, const ti_rollout_desc* desc, int32_t n_probes, uint64_t probe_seed, const float* x0,
                               const float* cond, int64_t B, float div_scale, float out_scale, int reverse_ode, float* out_path,
                               float* out_dlogp, int64_t* n_fevals);

/* ---- shared ------------------------------------------------------------------------------------------------------ */
/* Accepted and rejected step counts [B] (host) of every trajectory of the last TI_SCHEME_DOPRI5_TRAJ rollout on this handle
 * (torchdiffeq's per-solve counts of a batch-of-one run); TI_E_ARG if B differs from that rollout's batch. */
int ti_rollout_step_counts(ti_handle* h, int64_t* accepted, int64_t* rejected, int64_t B);
void ti_destroy(ti_handle* h);
/* Streams.  A handle enqueues all device work on ONE stream: its own (created non-blocking at create()) or, with
 * ti_set_stream(h, s, TI_STREAM_EXTERNAL), the caller's hipStream_t `s` -- where s == NULL then means the legacy null stream
 * (torch's default stream reports cuda_stream == 0).  TI_STREAM_OWN restores the handle's own stream (`s` is ignored).
 * TI_MEM_DEVICE inputs written by work on ANOTHER stream (a torch kernel that produced x0 / cond) are ordered with
 * ti_wait_stream(h, producer): the handle's stream then waits for everything enqueued on `producer` so far (NULL = the null
 * stream).  Every call returns after synchronising the handle's stream, so outputs need no further ordering. */
enum { TI_STREAM_OWN = 0, TI_STREAM_EXTERNAL = 1 };
int ti_set_stream(ti_handle* h, void* hip_stream, int mode);
int ti_wait_stream(ti_handle* h, void* producer_stream);
/* Pin the edge-row layout of a painn handle: TI_TEMPLATE_AUTO (from the batch size of each call, the default),
 * TI_TEMPLATE_THROUGHPUT, TI_TEMPLATE_LATENCY (directed edge rows sorted by destination) or TI_TEMPLATE_PAIR (pair-major rows:
 * the filter branch w(enc(|r_ij|)) of SE3Message, cpainn.py:283-289, is evaluated once per atom pair and shared by the edges i->j
 * and j->i; needs a symmetric graph, F <= 128 and TI_PREC_F32 / TI_PREC_F16X2, otherwise the request falls back to
 * TI_TEMPLATE_THROUGHPUT; the divergence / tangent entry points always use a directed layout).  Results are bit-identical
 * within one layout and agree to fp32 round-off across them, so a run sharded over ranks pins the layout it would use for the
 * GLOBAL batch and becomes independent of the rank count.  (The TI_TEMPLATE environment variable, read per call, overrides this.) */
enum { TI_TEMPLATE_AUTO = -1, TI_TEMPLATE_THROUGHPUT = 0, TI_TEMPLATE_LATENCY = 1, TI_TEMPLATE_PAIR = 2 };
int ti_painn_set_template(ti_handle* h, int which);
/* the layout ti_painn_drift / ti_painn_rollout would choose for a batch of B molecules (TI_TEMPLATE_THROUGHPUT / _LATENCY / _PAIR) */
int ti_painn_template_for(ti_handle* h, int64_t B);
/* Per-molecule edge sets over the handle's template.  mask [B][A]: bit s of mask[b*A + d] = edge s -> d exists in molecule b.
 * Template edges whose bit is clear contribute nothing to molecule b (drift, JVP, exact and Hutchinson divergence, every
 * rollout scheme, both dopri5 step controls); bits of pairs outside the template are ignored.  The mask is copied into the
 * handle and stays in force for later calls whose B equals its B (another B: TI_E_ARG); mask == NULL clears it.
 * Molecule indices are local to the call, like x0: a traj_offset shard passes its slice of the mask.  The pair layout is
 * eligible only while every molecule's set is symmetric over the template (checked here); a call on a handle pinned to
 * TI_TEMPLATE_PAIR with an asymmetric mask in force returns TI_E_UNSUPPORTED.  A NULL or non-painn handle, B < 1 with a
 * non-NULL mask, or an unknown mem: TI_E_ARG before any device work.  An all-ones mask gives the unmasked results bit for bit. */
int ti_painn_set_edge_mask(ti_handle* h, const uint32_t* mask, int64_t B, int mem);
/* Mixed-species batches: per-molecule atom counts, edge sets and edge types over the handle's template (A = the largest molecule).
 * n_atoms [B], each in 1..A: atoms a >= n_atoms[b] of molecule b are PAD atoms.  mask [B][A] as in ti_painn_set_edge_mask; NULL:
 * every template edge between real atoms.  The library clears every bit that touches a pad atom itself.  pair_type [B][A][A]
 * (bytes, 0..3): pair_type[(b*A + s)*A + d] is the type of the edge s -> d in molecule b; NULL: the template's types; entries of
 * absent edges are ignored.  This call and ti_painn_set_edge_mask write the same per-molecule graph state and the later call
 * replaces the earlier one completely (set_edge_mask: all n_atoms = A, template types); n_atoms == NULL clears the state.  `mem`
 * says where all three arrays live.  TI_E_ARG before any device work: a NULL or non-painn handle, B < 1, a count outside 1..A, a
 * type above 3 (host arrays; device arrays are checked after their copy), an unknown mem; a later call with another B: TI_E_ARG.
 * The pair layout is eligible only while every molecule's mask AND types are symmetric (TI_E_UNSUPPORTED on a handle pinned to it
 * otherwise, as for masks).
 *   Pad atoms in every output: a pad atom's drift (and tangent) is written as exactly +0 by the library, its coordinates in every
 *     out_path row are those of x0, it receives no EM noise, and with com_free_noise the centre of mass is taken over the
 *     n_atoms[b] real atoms.
 *   Independence from pad inputs: every result on real atoms (drift, JVP, exact and Hutchinson divergence, every rollout) is
 *     bit-identical whatever finite coordinates, directions and cond values the pad atoms carry, coinciding ones included: the
 *     kernels never see them.  The library evaluates the network on a copy in which pad atom a of molecule b sits at
 *     x[b][0] + (100 (a - n_atoms[b] + 1), 0, 0) with cond 0 (and tangent direction 0), every row that touches it switched off.
 *   Adaptive solvers: TI_SCHEME_DOPRI5 takes the error ratio and Hairer's initial step as the rms over the sum_b 3 n_atoms[b]
 *     real entries (torchdiffeq's norm of the reference's flat [N,3] state); TI_SCHEME_DOPRI5_TRAJ takes trajectory b's rms over
 *     its 3 n_atoms[b] entries (maxed with its dlogp entry, as before).  Its path, dlogp and step counts do not depend on what
 *     the other molecules of the call are: they are bit for bit those of a batch of the same B that holds only its species, on the
 *     same handle and pinned layout, with the molecule at the same index.  On TI_TEMPLATE_LATENCY (one molecule per row group) they
 *     are also those of any smaller batch and any index.  TI_TEMPLATE_THROUGHPUT and TI_TEMPLATE_PAIR pack several molecules into
 *     one row group and a molecule's per-atom sums follow its place in the group, as they do without masks: a batch that moves it
 *     to another place in its group agrees to fp32 round-off only (1e-6 absolute on a path), mixed species or not.  The same holds
 *     for the Hutchinson estimate below.
 *   Hutchinson: real component (a, c) of trajectory id traj_offset + b draws N(probe_seed, id, p, 3a + c) as before (the probes it
 *     would get alone); pad components are 0.  Exact divergence: the 3 n_atoms[b] real unit seeds are summed, pads are skipped.
 *   With every n_atoms[b] == A and pair_type == NULL every entry point returns the bits ti_painn_set_edge_mask(mask) returns. */
int ti_painn_set_molecules(ti_handle* h, const int32_t* n_atoms, const uint32_t* mask, const uint8_t* pair_type, int64_t B, int mem);
/* ---- observables: per-molecule collective variables (CVs), importance weights, weighted histograms ----------------------------
 * No reference FFI counterpart; what they compute is the reference's analysis layer: internal coordinates
 * (mdqm9/analysis/utils/mol_geometry.py compute_distance / compute_angle / compute_torsion, histogrammed by z_matrix.py:43-45 and
 * results_00031.py:140-149), the effective sample size (mdqm9/analysis/utils/ess.py:32-35) and the adw free-energy profile.
 * All of them run on the handle's stream and device, take a painn or an adw handle, compute in fp64 from the fp32 inputs, use no
 * atomics and repeat bit for bit; a per-molecule value does not depend on the other molecules of the batch, the batch-wide sums
 * (weights, histograms) are taken in an order fixed by B.  Arguments are validated before any device work.
 *
 * A CV descriptor is five int32 (kind, i, j, k, l); unused slots are ignored.  x [B,A,3] (painn) or [B,d] (adw):
 *   RMSD           minimal RMSD over PROPER rotations of molecule b to ref [A,3] over the atoms a with select[a] != 0 (select == NULL:
 *                  all), both sets centred over those atoms: sqrt(max(|x|^2 + |ref|^2 - 2 lambda, 0) / count), lambda the largest
 *                  eigenvalue of Horn's 4x4 quaternion matrix of the covariance (fixed-sweep Jacobi; rank-deficient covariances --
 *                  one or two atoms, collinear or planar sets -- included).  A mirror image does not give 0.  No selected atom: NaN.
 *   DIST(i,j)      |x_j - x_i|
 *   ANGLE(i,j,k)   the angle at j between j->i and j->k, radians in [0, pi]
 *   TORSION(i,j,k,l)  atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3)), b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k; radians in (-pi, pi]
 *   COORD(c)       adw handles only, and the only kind they take: component c of a particle, 0 <= c < d
 * Mixed-species batches (ti_painn_set_molecules in force, B equal to its B): RMSD runs over the real selected atoms of molecule b;
 * a descriptor that names a pad atom of molecule b yields NaN for that molecule; pad coordinates are never read.
 * TI_E_ARG: an index outside 0..A-1 (COORD: 0..d-1), an unknown kind, a geometric kind on an adw handle or COORD on a painn handle,
 * RMSD without ref, K < 1, a NULL buffer. */
enum { TI_OBS_RMSD = 0, TI_OBS_DIST = 1, TI_OBS_ANGLE = 2, TI_OBS_TORSION = 3, TI_OBS_COORD = 4 };
/* desc [K][5], ref [A,3] fp32 and select [A] int32 (both may be NULL): host memory.  x and out_cv [B,K] fp32: [host|device] by mem. */
int ti_obs_cv(ti_handle* h, const int32_t* desc, int32_t K, const float* ref, const int32_t* select, const float* x, int64_t B,
              float* out_cv, int mem);
/* Importance weights of logw [B] fp32 [host|device] (e.g. -dlogp plus an energy term): m = max logw, w = exp(logw - m), two-pass
 * fixed-order fp64 sums; out_w [B] fp32 [host|device] = w / sum w (may be NULL); *out_ess (host) = (sum w)^2 / sum w^2, calc_ESS of
 * the reference.  A non-finite entry: TI_E_NAN, the message names the first such index. */
int ti_obs_weights(ti_handle* h, const float* logw, int64_t B, float* out_w, double* out_ess, int mem);
/* Weighted histogram of values[i * stride], i < B (fp32 [host|device]; a column of a [B,K] CV array has stride K), over n_bins equal
 * bins on [lo, hi), 1 <= n_bins <= 256, edges e_k = lo + ((hi - lo) k) / n_bins in fp64; a value equal to an interior edge goes to
 * the upper bin.  Weights: the normalised exp(logw) of ti_obs_weights (same refusal), or 1 / B with logw == NULL.  out_hist
 * [n_bins] and out_tails [3] (host, double): the weight per bin; the weight below lo, at or above hi, and of non-finite values (which
 * are not binned) -- sum(out_hist) + sum(out_tails) = 1 to round-off.  n_bins outside 1..256 or hi <= lo: TI_E_ARG. */
int ti_obs_hist(ti_handle* h, const float* values, int64_t stride, const float* logw, int64_t B, int32_t n_bins, double lo, double hi,
                double* out_hist, double* out_tails, int mem);
/* Bootstrap of the estimators the reference's analysis reports with a 95 % interval (mdqm9/analysis/results_00031.py gen_ess_*,
 * gen_free_energy_*), after its IQR outlier filter (utils/sensititvity.py filter_iqr).  v_i = logw[i] = -phi_i, m = max v,
 * w_i = exp(v_i - m); fp64 arithmetic on the fp32 inputs.  Over a multiset S of sample indices:
 *   TI_BOOT_ESS    (sum_S w)^2 / sum_S w^2              calc_ESS
 *   TI_BOOT_TFEP   -(m + ln(sum_S w / |S|))             calc_tfep_dF with unit weights: -ln <exp(-phi)>
 *   TI_BOOT_MEAN   -(sum_S v) / |S|                     calc_bg_dF: <phi>
 * Filter: q25, q75 by numpy's default (linear) percentile rule -- at position h = (|S| - 1) p the value x_[h] + (h - [h]) (x_[h]+1 -
 * x_[h]) of the sorted x -- iqr = q75 - q25, keep q25 - k iqr < x < q75 + k iqr; x = w for ESS and TFEP (the reference filters
 * exp(v); the rule is scale invariant, so the kept set is the same), x = v for MEAN.  Nothing kept (always so for one sample or a
 * constant sample, whose iqr is 0): NaN.
 *   TI_BOOT_FILTER_NONE      the population is all n samples
 *   TI_BOOT_FILTER_ONCE      (gen_ess_ti, gen_ess_bg) the sample is filtered once; the survivors, in index order, are the population of
 *                            the point estimate and of every resample
 *   TI_BOOT_FILTER_RESAMPLE  (gen_free_energy_*) the point estimate is that of the once-filtered sample; every resample draws from all
 *                            n samples and is filtered by its own quartiles
 * Draws.  idx == NULL: a resample draws n_draw population indices (n_draw == 0: as many as the population holds).  Draw j of global
 * resample R = first + r is  (u * n_pop) >> 64  with the 64-bit u = o[2 (j & 1)] | o[2 (j & 1) + 1] << 32 of the four 32-bit words
 *   o = Philox4x32-10(counter = (j >> 1, R & 0xffffffff, R >> 32, 0x424f4f54), key = (seed & 0xffffffff, seed >> 32)),
 * so the estimate of resample R depends on (seed, R, the data, the mode) only -- not on n_boot, on first beyond R, or on the GPU
 * that computes it.  idx != NULL: row r holds the n_draw >= 1 population indices of resample r (the reference's own np.random.choice
 * rows; with RESAMPLE, n_draw = the kept count and indices below it reproduce the reference drawing only len(filtered) indices over
 * the unfiltered arrays).  An index row gives the same bits whether it came from the generator or from idx.  Every sum runs in an
 * order fixed by n_draw; a call repeats bit for bit.
 * out [4] (host): the point estimate; the (1 - level) / 2 and (1 + level) / 2 percentiles of the n_boot estimates by the same linear
 * rule (NaN with n_boot == 0 or a NaN estimate, as np.percentile); the kept count of the point estimate.  out_boot [n_boot] fp64
 * (may be NULL): the estimates.
 * TI_E_ARG, before anything is written: a NULL handle, logw, d or out; n < 1 or n > 2^31 - 1; an unknown estimator, filter or mem; a
 * filter with k not finite or <= 0; level outside (0, 1); n_boot < 0 or > 2^20; n_draw < 0; idx with n_draw < 1; an idx entry
 * outside the population (found on the device; the entry is not followed).  TI_E_NAN: a non-finite logw, as in ti_obs_weights. */
enum { TI_BOOT_ESS = 0, TI_BOOT_TFEP = 1, TI_BOOT_MEAN = 2 };
enum { TI_BOOT_FILTER_NONE = 0, TI_BOOT_FILTER_ONCE = 1, TI_BOOT_FILTER_RESAMPLE = 2 };
#define TI_BOOT_DOMAIN 0x424f4f54u   /* the fourth counter word of the draws ("BOOT") */
#define TI_BOOT_MAX_RESAMPLES (1 << 20)
typedef struct {
    int32_t  estimator, filter;
    double   k;        /* IQR multiple, finite and > 0; ignored with FILTER_NONE */
    double   level;    /* 0 < level < 1; the interval is the (1-level)/2 and (1+level)/2 percentiles */
    int64_t  n_boot;   /* >= 0; 0 = point estimate only */
    int64_t  first;    /* resample r of this call is global resample first + r (lets ranks split a bootstrap) */
    uint64_t seed;
} ti_boot_desc;
/* logw [n] fp32, idx [n_boot, n_draw] int32 or NULL, out_boot [n_boot] fp64 or NULL: [host|device] by mem.
   out [4] host double: point estimate, lower, upper, kept count of the point estimate. */
int ti_obs_bootstrap(ti_handle* h, const float* logw, int64_t n, const ti_boot_desc* d,
                     const int32_t* idx, int64_t n_draw, double* out, double* out_boot, int mem);
/* Gram matrices of random Fourier features over bootstrap resamples: the O(m p^2) part of reversible generator EDMD (the reference's
 * gedmd/rff.py spectral_analysis_rff_generator, bootstrapped by adw/analysis/reweight_gedmd.py bootstrap_eigenvalues).  With
 * theta_nk = sum_i x_ni omega_ik (fp64 on the fp32 values, i ascending), M_nk = exp(-i theta_nk) = c_nk - i s_nk and weights
 * w_n = exp(logw_n - max logw) (logw == NULL: 1), the Gram matrix of a multiset S of sample indices is
 *   G_kl = sum_S w conj(M_k) M_l:   Re G_kl = sum_S w (c_k c_l + s_k s_l),   Im G_kl = sum_S w (s_k c_l - c_k s_l),
 * an fp64 contraction on the matrix cores.  The singular values of M^H (weighted by sqrt w) are sqrt(eig G) and its left singular
 * vectors are the eigenvectors of G, so the whole spectral analysis is host algebra on the p x p result.
 * values: row n holds the d components x_n0 .. x_n,d-1 at values[n * stride]; stride >= d (an adw state [B,d], or columns of a
 * [B,K] CV array).  omega [d,p] fp64, host.  1 <= d <= 16, 1 <= p <= 128.  The call keeps a table of cos / sin of 2 n P doubles,
 * P = p rounded up to 16: n P > 2^27 (2 GiB) is refused with TI_E_ALLOC.
 * out [1 + n_boot, p, p, 2] fp64 (re, im): row 0 is the point estimate, S = all n samples in order; row 1 + r is resample r.  Draws are
 * exactly those of ti_obs_bootstrap: idx == NULL: n_draw population indices (0: n) per resample from Philox with counter
 * (j >> 1, R, TI_BOOT_DOMAIN) and key seed, R = first + r; idx != NULL: row r of idx [n_boot, n_draw].
 * Every output is exactly Hermitian (the lower triangle is the stored conjugate of the upper, Im of the diagonal is 0).  A row's draws
 * are cut into segments of 8192; every segment is summed in draw order and the segments are added in order, without atomics: a row
 * is a function of (its draws, the data, omega, n_draw) only -- not of n_boot, of first beyond R, of generator versus idx, of mem, or
 * of how many rows share a launch -- and a call repeats bit for bit.
 * TI_E_ARG, before any device work: a NULL handle, values, omega, g or out; an unknown mem; n < 1 or n > 2^31 - 1; d or p out of range;
 * stride < d; a non-finite omega; n_boot < 0 or > TI_BOOT_MAX_RESAMPLES; n_draw < 0; idx with n_draw < 1.  TI_E_ARG with out untouched:
 * an idx entry outside 0..n-1 (found on the device; the entry is not followed).  TI_E_NAN: a non-finite logw, naming its index. */
typedef struct { int32_t d, p; int64_t n_boot, first; uint64_t seed; } ti_gram_desc;
/* values [n rows, stride] fp32, logw [n] fp32 or NULL, idx [n_boot, n_draw] int32 or NULL, out fp64: [host|device] by mem. */
int ti_obs_rff_gram(ti_handle* h, const float* values, int64_t stride, int64_t n, const double* omega, const float* logw,
                    const ti_gram_desc* g, const int32_t* idx, int64_t n_draw, double* out, int mem);
/* ti_obs_rff_gram for 1 <= p <= TI_GRAM_WIDE_MAX_P (the molecule study's p = 300 and the model-selection grids up to p = 1000 of the
 * reference's mdqm9/analysis/gedmd.py and the two model_selection.py scripts): the arguments, the output layout [1 + n_boot, p, p, 2], the draws, the
 * mem modes, the staging, the feature-table cap n P <= 2^27 and every refusal are those of ti_obs_rff_gram; only the range of p differs.
 * p <= 128 runs the kernels of ti_obs_rff_gram and returns the bits it returns.  Beyond that the P / 16 column tiles are cut into
 * panels of 8 tiles (the last may be narrower) and one workgroup per (resample row, segment of 8192 draws, panel pair I <= J)
 * accumulates the pair's tiles -- the upper triangle of a diagonal pair, all of an off-diagonal one -- with both panels of the 16
 * gathered draws in LDS.  A 16 x 16 tile is summed exactly as ti_obs_rff_gram sums it (four draws per step in draw order, the chunk and
 * segment boundaries at the same draws), so a tile of the result holds the bits ti_obs_rff_gram gives for that pair of column tiles
 * of omega.  Every output is exactly Hermitian, Im of the diagonal is 0.  No atomics.
 * A row is a function of (its draws, the data, omega, n_draw) only.  It does not depend on n_boot, on first beyond R, on generator
 * versus idx, on mem, or on rows per launch.  A call repeats bit for bit.
 * An out-of-range idx entry is TI_E_ARG with out untouched.  A non-finite logw is TI_E_NAN with its index. */
#define TI_GRAM_WIDE_MAX_P 1024
int ti_obs_rff_gram_wide(ti_handle* h, const float* values, int64_t stride, int64_t n, const double* omega, const float* logw,
                         const ti_gram_desc* g, const int32_t* idx, int64_t n_draw, double* out, int mem);
/* Batched complex-Hermitian fp64 eigensolver on the device: numpy.linalg.eigh(A, UPLO="U") of n_mat matrices of order n <= 64, one
 * 256-thread workgroup per matrix, A and the accumulated eigenvector matrix V both in LDS (2 m m 16 bytes plus small tables, m = n
 * rounded up to even: 128 KiB at n = 64; n <= 50 leaves room for two workgroups per CU).
 * Only the upper triangle of a matrix is read; the real part is taken on the diagonal and the lower triangle is taken to be the
 * conjugate.  w is ascending; exactly equal eigenvalues are ordered by the diagonal position they converged at.  Column k of v is a
 * unit eigenvector for w[k]; its phase is unspecified.
 * Method: parallel cyclic two-sided Jacobi.  A sweep is the m - 1 rounds of the round-robin tournament: slot 0 holds index 0, slot
 * k >= 1 holds index 1 + (k - 1 + r) mod (m - 1) in round r, slot i is paired with slot m - 1 - i; a pair that contains the pad index
 * (odd n) is skipped.  The rotation of a pair (p, q), p < q, with b = A[p,q] is skipped when |b| <= 2^-53 scale, scale the largest
 * |A[k,k]| of the input; otherwise tau = (A[q,q] - A[p,p]) / (2 |b|), t = sign(tau) / (|tau| + sqrt(1 + tau^2)) with sign(0) = +1,
 * c = 1 / sqrt(1 + t^2), s = t c, e = conj(b) / |b| and U = [[c, s], [-s e, c e]] on columns (p, q).  Every rotation of a round is
 * computed from the matrix as it stands at the start of that round; then A <- A U and V <- V U on all the round's column pairs, then
 * A <- U^H A on its row pairs; the annihilated entries are set to exactly 0 and the imaginary parts of the touched diagonal entries
 * to 0.  fp64 hypot, sqrt and division throughout.  The iteration stops after the first sweep in which no pair was rotated; sweeps
 * [n_mat] (may be NULL) counts that sweep too: 1 for a diagonal matrix.
 * No atomics.  The result is a function of the matrix alone -- not of its position in the batch, of n_mat, of mem, or of how a batch
 * is cut into launches -- and a call repeats bit for bit.  Results go to a buffer of the handle first and reach w, v and sweeps only
 * when the whole call succeeded.
 * TI_E_ARG, before any device work: a NULL handle, a or w; an unknown mem; n outside 1..TI_EIGH_MAX_N; n_mat outside
 * 1..TI_BOOT_MAX_RESAMPLES + 1.  TI_E_NAN, nothing written: a non-finite entry in the triangle that is read (found on the device;
 * the first such matrix is named).  TI_E_UNSUPPORTED, nothing written: a matrix still rotating after 64 sweeps (named). */
#define TI_EIGH_MAX_N 64
/* a [n_mat, n, n, 2] fp64 (re, im), w [n_mat, n] fp64, v [n_mat, n, n, 2] fp64 or NULL, sweeps [n_mat] int32 or NULL: [host|device] by mem */
int ti_obs_eigh(ti_handle* h, const double* a, int64_t n_mat, int32_t n, double* w, double* v, int32_t* sweeps, int mem);
/* The p x p algebra of reversible generator EDMD on the device, per Gram matrix G (as ti_obs_rff_gram writes them; the upper triangle
 * is read, as in ti_obs_eigh): the eigenpairs of G in descending order, s = sqrt(max(lambda, 0)), r = max(#{k : s_k / s_0 >= tol}, nev)
 * (a division, then the comparison), L = U[:, :r] / s[:r], ML_kl = -a/2 K_kl G_kl with K = omega^T omega (formed once per call on the
 * host in fp64, i ascending), R = L^H ML L, the eigenpairs of its Hermitian part (real diagonal) from the same Jacobi kernel at order
 * r; ev = the last nev eigenvalues in ascending order, vec = L Wi[:, -nev:], rank = r.  Limits: 1 <= p <= 64 (a larger p returns
 * TI_E_UNSUPPORTED: the host route, observables.gedmd_spectrum(solver="host"), has no such limit), 1 <= d <= 16, 1 <= nev <= p, a
 * finite, tol finite and >= 0, omega finite, n_mat as for ti_obs_eigh; all checked before the handle is looked at.  A Gram matrix
 * whose largest eigenvalue is not positive, or whose kept s contains 0 (tol = 0 on a rank-deficient G), gives NaN in that matrix's ev
 * and vec; it is not an error.  TI_E_NAN (a non-finite Gram entry) and TI_E_UNSUPPORTED (64 sweeps) as in ti_obs_eigh, nothing written.
 * Deterministic in the same sense as ti_obs_eigh. */
typedef struct { int32_t d, p, nev, reserved; double a, tol; } ti_gedmd_desc;   /* 32 bytes, reserved = 0 */
/* gram [n_mat, p, p, 2] fp64, ev [n_mat, nev] fp64, vec [n_mat, p, nev, 2] fp64 or NULL, rank [n_mat] int32 or NULL: [host|device] by mem;
   omega [d, p] fp64, host */
int ti_obs_gedmd_spectrum(ti_handle* h, const double* gram, int64_t n_mat, const double* omega, const ti_gedmd_desc* g,
                          double* ev, double* vec, int32_t* rank, int mem);
/* ti_obs_eigh for orders up to TI_EIGH_WIDE_MAX_N: the arguments, the triangle that is read, the order of w, the staging, the mem modes
 * and the refusals are those of ti_obs_eigh; only the range of n differs.  n <= 64 runs the kernel of ti_obs_eigh and returns the
 * bits it returns.  Beyond that A and V live in buffers of the handle in global memory and the method is a blocked two-sided Jacobi:
 *   thr = 2^-53 max_k |A[k,k] of the input|, of the whole matrix.  Blocks are 32 indices wide: nb = ceil(n / 32) of them, the last may
 *   be narrow; mb = nb rounded up to even.  An outer sweep is the mb - 1 rounds of ti_obs_eigh's tournament over the mb block slots
 *   (slot 0 holds block 0, slot k >= 1 block 1 + (k - 1 + r) mod (mb - 1), slot i meets slot mb - 1 - i); a pair that holds the pad
 *   block is skipped.  The block pairs of a round are disjoint and every one is formed from the matrix as it stands at the start of
 *   the round.
 *   The visit of a block pair I < J: S = A[idx, idx] on the <= 64 indices idx of I then J.  ONE sweep of ti_obs_eigh's cyclic Jacobi
 *   is applied to S in LDS -- all rounds of the tournament over its order (rounded up to even), the same rotation formulas, exact
 *   zeros and real diagonal -- with the threshold thr above, not one derived from S; U is the product of its rotations, accumulated
 *   from the identity.  Nothing is sorted.  Then, for all pairs of the round, A[:, idx] <- A[:, idx] U and V[:, idx] <- V[:, idx] U,
 *   then A[idx, :] <- U^H A[idx, :], and A[idx, idx] becomes what the inner sweep left.  The products are real fp64 products on the matrix
 *   cores (v_mfma_f64_16x16x4_f64, as in ti_obs_rff_gram), summed over the indices of idx in ascending order, four per instruction:
 *   re += x.re u.re, re += (-x.im) u.im, im += x.re u.im, im += x.im u.re, in this order (x conjugated first where U^H is applied).
 *   A pair whose inner sweep rotated nothing leaves the matrix as it is.
 *   The iteration ends after the first outer sweep in which no visit rotated; sweeps counts that sweep too.  w is the diagonal in
 *   ascending order, equal values by position, v the columns of V in that order.
 * The host reads one status word per matrix after every outer sweep; workgroups of a finished matrix exit at once.  No atomics, no
 * waiting of one workgroup on another: kernel boundaries on the handle's stream are the only synchronisation.  A launch takes
 * ti_obs_eigh_wide_launch_max(n) matrices.  The result is a function of the matrix alone, as for ti_obs_eigh.
 * TI_E_ARG, before any device work: as ti_obs_eigh with n outside 1..TI_EIGH_WIDE_MAX_N.  TI_E_NAN and TI_E_UNSUPPORTED (64 outer
 * sweeps) as ti_obs_eigh, nothing written. */
#define TI_EIGH_WIDE_MAX_N 1024
int ti_obs_eigh_wide(ti_handle* h, const double* a, int64_t n_mat, int32_t n, double* w, double* v, int32_t* sweeps, int mem);
/* Matrices per launch of the blocked solver at order n: min(512, 2^31 / (32 n^2)), A and V at 32 n^2 bytes a matrix; 0 for n outside
 * 1..TI_EIGH_WIDE_MAX_N.  Needs no handle. */
int64_t ti_obs_eigh_wide_launch_max(int32_t n);
/* ti_obs_gedmd_spectrum for 1 <= p <= TI_EIGH_WIDE_MAX_N: the same arguments, definitions, outputs and refusals; only the range of p
 * differs.  p <= 64 is ti_obs_gedmd_spectrum itself and returns its bits.  Beyond that both solves are ti_obs_eigh_wide's (a reduced
 * matrix of order r <= 64 goes through ti_obs_eigh's kernel), and L, T = ((-a/2) K o G) L and R = L^H T are global-memory products of
 * plain fp64 multiply-adds, every entry summed over its index in ascending order. */
int ti_obs_gedmd_spectrum_wide(ti_handle* h, const double* gram, int64_t n_mat, const double* omega, const ti_gedmd_desc* g,
                               double* ev, double* vec, int32_t* rank, int mem);
/* Force-field energies: the reduced potential energies the weight estimators above take (E0s, E1s of the reference's
 * mdqm9/analysis/utils/ess.py:8-10), for what mdqm9/analysis/eval_energy.py evaluates one conformation at a time through OpenMM:
 * the HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce and NonbondedForce (NoCutoff, vacuum) of
 * forcefield.createSystem(topology), times 1 / (k_B N_A T).  Energies in kJ/mol, lengths in nm, angles in radians.  Positions are
 * p = (double)x * to_nm.  The four term sums of a molecule:
 *   bond     (i, j), (r0, k)                  E = k (r - r0)^2 / 2,  r = |p_j - p_i|
 *   angle    (i, j, k), (theta0, k)           E = k (theta - theta0)^2 / 2,  theta the TI_OBS_ANGLE angle at j as acos of the cosine
 *                                             u.v / (|u| |v|) clamped to [-1, 1] (u = p_i - p_j, v = p_k - p_j)
 *   torsion  (i, j, k, l), (n, phase, k)      E = k (1 + cos(n phi - phase)),  phi the TI_OBS_TORSION angle, n an integer in 1..6
 *   pair     row i (2A - i - 1) / 2 + (j - i - 1) of the dense table of all A (A - 1) / 2 pairs i < j, (qq, sigma, eps)
 *                                             E = 4 eps ((sigma / r)^12 - (sigma / r)^6) + coulomb qq / r,  r = |p_j - p_i|
 *            A row with qq == 0 and eps == 0 is skipped: it contributes exactly 0 and is never evaluated (the 1-2 and 1-3 exclusions
 *            arrive in that form).  The Lennard-Jones part is formed as 4 eps s (s - 1), s = (sigma / r)^6, and only with eps > 0 and
 *            sigma > 0; the Coulomb part only with qq != 0.  r = 0: a pair with a Lennard-Jones part is +inf (the wall wins over an
 *            attractive charge product), a pair of charges alone is coulomb qq / 0.
 * ti_obs_ff_set copies a force field for the handle's species into a painn handle (an adw handle: TI_E_ARG).  All tables are host
 * memory, parameters fp64, indices int32: bond_idx [n_bonds][2], bond_par [n_bonds][2], angle_idx [n_angles][3], angle_par
 * [n_angles][2], torsion_idx [n_torsions][4], torsion_par [n_torsions][3] (n as a double holding an integer), pair_par [n_pairs][3];
 * a table whose count is 0 may be NULL.  desc == NULL clears the force field.  One force field is one species: a handle with
 * ti_painn_set_molecules in force gets TI_E_UNSUPPORTED (here and in ti_obs_ff_energy).  TI_E_ARG, before any device work and with
 * the force field in force left as it was: a count below 0 or above its TI_FF_MAX_* cap, n_pairs != A (A - 1) / 2 (so A <= 25), an
 * index outside 0..A-1, a repeated atom within one term, a non-finite parameter or coulomb, sigma < 0 or eps < 0, n not an integer
 * in 1..6, a NULL table with a positive count. */
#define TI_FF_MAX_BONDS 64
#define TI_FF_MAX_ANGLES 128
#define TI_FF_MAX_TORSIONS 512
#define TI_FF_MAX_PAIRS 300          /* A = 25; every table and four molecules' coordinates take about 25 KB of LDS */
#define TI_FF_GAS_CONSTANT 0.00831446261815324      /* R = k_B N_A in kJ / (mol K) */
typedef struct { int32_t n_bonds, n_angles, n_torsions, n_pairs; double coulomb; /* 138.935456: OpenMM's ONE_4PI_EPS0 */ } ti_ff_desc;
int ti_obs_ff_set(ti_handle* h, const ti_ff_desc* desc, const int32_t* bond_idx, const double* bond_par, const int32_t* angle_idx,
                  const double* angle_par, const int32_t* torsion_idx, const double* torsion_par, const double* pair_par);
/* x [B,A,3] fp32 and T [B] fp32 (kelvin, one per molecule; NULL: none) and out_e [B], out_terms [B,4] fp64 (may be NULL):
 * [host|device] by mem.  out_terms[b] = the bond, angle, torsion and pair sums of molecule b in kJ/mol, each divided by
 * R T_b (R = TI_FF_GAS_CONSTANT, the product in fp64) when T is given; out_e[b] = ((bond + angle) + torsion) + pair of those four.
 * One wave per molecule, four molecules per 256-thread workgroup; a workgroup stages the tables in LDS once and loops over its
 * molecules, whose positions go to LDS as fp64 nm.  Lane l adds terms l, l + 64, ... of a table in that order, the 64 lane sums are
 * combined by a fixed butterfly; fp64 sqrt, acos, atan2, cos and division; no atomics.  A molecule's outputs are a function of its
 * coordinates, to_nm, T_b and the tables only -- not of its place in the batch, of B, of mem, or of how the batch is cut into
 * workgroups -- and a call repeats bit for bit.  Degenerate geometry is not an error: see r = 0 above; a NaN coordinate gives NaN
 * for that molecule only.
 * TI_E_ARG, nothing written: a NULL or adw handle, no force field set, B < 0, a NULL x or out_e with B > 0, an unknown mem, a
 * non-finite to_nm, T_b <= 0 or not finite (found on the device; the message names the first such index). */
int ti_obs_ff_energy(ti_handle* h, const float* x, int64_t B, double to_nm, const float* T, double* out_e, double* out_terms, int mem);
/* The analytic forces of the same force field: out_f[b,a,c] = -dE_b / d(p[b,a,c]) in kJ / (mol nm) at p = (double)x * to_nm, and with
 * out_e != NULL the energy of the same pass ((bond + angle) + torsion) + pair; with T both are divided by R T_b.  x [B,A,3] fp32,
 * T [B] fp32 or NULL, out_f [B,A,3] fp64, out_e [B] fp64 or NULL: [host|device] by mem.  Per term (u, v, b1, b2, b3, m = b1 x b2, n = b2 x b3 as above):
 *   bond     on j: -k (r - r0) (p_j - p_i) / r; on i its negative
 *   angle    through d theta / d cos = -1 / sin theta, sin theta = sqrt((1 - cos)(1 + cos)) of the clamped cosine:
 *            on i: k (theta - theta0) / (sin theta |u|) (v / |v| - cos u / |u|), on k the same with u and v exchanged, on j minus both
 *   torsion  k n sin(n phi - phase) d phi / dx with d phi / dx1 = -|b2| m / |m|^2, d phi / dx4 = |b2| n / |n|^2,
 *            d phi / dx2 = -(1 + b1.b2 / |b2|^2) d phi / dx1 + (b3.b2 / |b2|^2) d phi / dx4,
 *            d phi / dx3 = -(1 + b3.b2 / |b2|^2) d phi / dx4 + (b1.b2 / |b2|^2) d phi / dx1 (no division by sin phi)
 *   pair     on i: (24 eps s (2 s - 1) / r^2 + coulomb qq / r^3) (p_i - p_j), s = (sigma / r)^6, under the energy's rules for which
 *            part exists and which rows are evaluated; on j its negative
 * r = 0, a collinear angle, collinear b1, b2 or b2, b3 give a non-finite force for that molecule only; a NaN coordinate gives NaN for
 * its molecule only.  One wave per molecule, no atomics, no contraction: an atom's component is the running sum of its bonded
 * contributions in the order bonds, angles, torsions, ascending term index, plus its pair force, which is the sum over partners
 * 0 .. h-1 plus the sum over partners h .. A-1 (h = (A + 1) / 2), each ascending.  A molecule's outputs are a function of its
 * coordinates, to_nm, T_b and the tables only, and a call repeats bit for bit.  out_e is not promised to equal ti_obs_ff_energy bit
 * for bit.  Refusals: those of ti_obs_ff_energy in its order, nothing written. */
int ti_obs_ff_forces(ti_handle* h, const float* x, int64_t B, double to_nm, const float* T, double* out_f, double* out_e, int mem);
/* The masses [A] (host memory, amu) of the species of the force field in force, for ti_obs_ff_langevin.  TI_E_ARG, the masses in
 * force left alone: no force field, a mass that is not finite and > 0.  m == NULL clears them; ti_obs_ff_set clears them too. */
int ti_obs_ff_set_masses(ti_handle* h, const double* m);
/* Langevin dynamics of B replicas of the species under the force field in force, OpenMM's "middle" discretisation; units nm, ps, amu,
 * kJ/mol.  Step s of the call has the global index step_offset + s:
 *   v += dt f(x) / m;  x += (dt / 2) v;  v = a v + sqrt((1 - a^2) R T_b / m) xi;  x += (dt / 2) v,   a = exp(-friction dt)
 * xi[a,c] = the Philox normal (seed, id_b, step_offset + s, 3a + c) of TI_SCHEME_EM as the velocity loss draws it (oracle.normal bit
 * for bit; the step index enters through its low 32 bits), promoted to fp64; id_b = ids[b] or traj_offset + b.  friction == 0:
 * a = 1, no draw, plain leapfrog.  draw_velocities: vel is not read; v[a,c] = sqrt(R T_b / m_a) times the normal (seed, id_b,
 * step_offset, 3A + 3a + c).  One wave per replica; positions, velocities and forces stay in LDS as fp64 for a whole launch; the host
 * cuts the call into launches of at most steps_per_launch steps (0: TI_MD_DEFAULT_STEPS_PER_LAUNCH), the state passes through global
 * memory exactly and the noise is keyed by the global step, so the cut does not change a bit, and neither does a call chained from
 * two with step_offset advanced.  The forces are those of ti_obs_ff_forces (one body).
 * Frames: n_frames = n_steps / stride (0 with stride == 0); after every stride-th step of the call out_frames[b,k] = (x - mean of x
 * over the atoms, an fp64 sum in atom order) / to_nm rounded once to fp32, out_epot[b,k] the potential energy there in kJ/mol,
 * out_ekin[b,k] = sum m v^2 / 2 of the velocities there.  The state itself is never centred.
 * pos, vel [B,A,3] fp64 in/out, T [B] fp32, ids [B] int64 or NULL, out_frames [B,n_frames,A,3] fp32, out_epot, out_ekin
 * [B,n_frames] fp64 (each may be NULL): [host|device] by mem.  A replica whose positions or velocities turn non-finite stops
 * advancing; the call then returns TI_E_NAN naming the first such replica and the launch, pos and vel are not written (frames in
 * device memory may be partly written).  One wait for the verdict; a host call waits once more for its results.
 * TI_E_ARG before any device work: a NULL or adw handle, unknown mem, NULL d, pos or T, NULL vel without draw_velocities, dt <= 0 or
 * not finite, friction < 0 or not finite, a negative n_steps, stride, step_offset or steps_per_launch, stride > 0 with every output
 * NULL, B < 1, to_nm 0 or not finite, no force field, no masses.  TI_E_UNSUPPORTED: ti_painn_set_molecules in force.  TI_E_ARG with
 * nothing written: T_b <= 0 or not finite (found on the device as ti_obs_ff_energy finds it). */
#define TI_MD_DEFAULT_STEPS_PER_LAUNCH 1024
typedef struct {
    double dt;               /* ps, > 0 */
    double friction;         /* 1/ps, >= 0; 0 = no thermostat (NVE) */
    int64_t n_steps;         /* >= 0 */
    int64_t stride;          /* a frame after every stride-th step; 0 = no frames */
    int64_t step_offset;     /* first step's index, for chained calls */
    int64_t traj_offset;     /* replica b has id traj_offset + b unless ids is given */
    uint64_t seed;
    int32_t draw_velocities; /* 1: vel is drawn from N(0, R T_b / m_a) before the first step and not read */
    int32_t steps_per_launch;/* 0 = default; > 0: the host cuts the call into launches of at most this many steps */
} ti_md_desc;
int ti_obs_ff_langevin(ti_handle* h, const ti_md_desc* d, double* pos, double* vel, const float* T, const int64_t* ids, int64_t B,
                       double to_nm, float* out_frames, double* out_epot, double* out_ekin, int mem);
/* Replica exchange: the Langevin dynamics of ti_obs_ff_langevin with Metropolis exchanges of neighbouring rungs of a temperature
 * ladder in between.  B = n_ladders * K rows, K = n_rungs; row l K + k is rung k of ladder l, and T[l K + k] stays the temperature
 * of that row for ever: a row is a temperature, what moves is the configuration.  pos, vel, T, ids, the frames and their energies
 * mean what they mean in ti_obs_ff_langevin, and the steps between two attempts are its launches, unchanged: the host cuts the call
 * at every attempt and after every steps_per_launch steps since the last cut.
 * An attempt follows global step count g (steps step_offset .. g - 1 done, g > step_offset) whenever g % exchange_every == 0; its
 * index is n = g / exchange_every, so one call and any chain of calls with step_offset advanced run the same attempts.  A frame due
 * at the same g is written first: it shows the state before the exchange.  Attempt n pairs the rungs (k, k + 1) with
 * k % 2 == n % 2 and k + 1 < K.  E_k = ((bond + angle) + torsion) + pair of the force pass at the fp64 state of row l K + k: the bits
 * out_epot reports for a frame at that step.  In fp64 without contraction:
 *   beta_k = 1 / (R (double)T_k),  delta = (beta_k - beta_k1) (E_k - E_k1),  k1 = k + 1
 *   u = the uniform ((w >> 8) + 0.5) 2^-24 (fp32) of word k & 3 of Philox4x32-10 under the key seed on the counter
 *       {lo32(ladder id), hi32(ladder id), (uint32_t)n, TI_REMD_DOMAIN + (k >> 2)}, ladder id = ladder_ids[l] or l
 *       (the noise and velocity draws of the same seed have a fourth word below 64)
 *   accept iff E_k and E_k1 are finite, neither row has stopped, and delta >= 0 or (double)logf(u) < delta
 * (logf: the host libm's, as the Philox normals evaluate it).  On acceptance the rows exchange pos, vel and walker, the velocities
 * rescaled in fp64 at the positions' time.  The "middle" scheme stores v = w - h, w the velocity at the positions and
 * h = (dt / 2) f(x) / m half a kick (its step starts with the whole kick), and it is w that is Maxwell-distributed and independent
 * of x.  With h_k the half kick of the configuration at row k, of the same force pass as E_k:
 *   row k  receives (v(k1) + h_k1) sqrt((double)T_k / (double)T_k1) - h_k1,
 *   row k1 receives (v(k)  + h_k)  sqrt((double)T_k1 / (double)T_k) - h_k.
 * (Rescaling the stored v alone leaves the cold rung of a harmonic bond 16 % short of its positional variance at dt = 1 fs,
 * friction 0.1 / ps and an exchange every 14 steps: profiles/remd_mutations.txt.)
 * walker [B] int32, in and out: the rung at which the configuration now at row b started; NULL: the identity, nothing returned.
 * out_walker [n_attempts][B]: walker after each attempt of the call; out_counts [n_ladders][K-1][2] int64: the attempts and
 * acceptances of pair (k, k + 1) in this call; n_attempts = (step_offset + n_steps) / exchange_every - step_offset / exchange_every.
 * ladder_ids [n_ladders] int64 or NULL.  All arrays [host|device] by mem; each output may be NULL.
 * One wave per pair, four pairs per workgroup, one launch per attempt; the energies stay on the chip; each pair's counts and labels
 * are owned by one wave (ordinary stores, no atomics).  A row's outputs are a function of its ladder's inputs only: repeating the
 * call, cutting it into launches, chaining it, moving a ladder within the batch and host against device memory do not change a bit,
 * and a call in which no attempt falls is ti_obs_ff_langevin bit for bit.
 * A replica stopped by the Langevin kernel takes part in no further pair; the call returns TI_E_NAN as ti_obs_ff_langevin does and
 * pos, vel and walker are not written.  Refusals: those of ti_obs_ff_langevin in its order; then TI_E_ARG before any device work for
 * r == NULL, n_rungs < 2 or > TI_REMD_MAX_RUNGS, B % n_rungs != 0, exchange_every < 1, reserved != 0, a walker entry outside
 * 0 .. K-1 (host memory; in device memory it is found on the device like a bad T, nothing written). */
#define TI_REMD_MAX_RUNGS 64
#define TI_REMD_DOMAIN 0x52454D44u     /* fourth Philox counter word of the exchange draws */
typedef struct { int32_t n_rungs; int32_t reserved; int64_t exchange_every; } ti_remd_desc;
int ti_obs_ff_remd(ti_handle* h, const ti_md_desc* d, const ti_remd_desc* r, double* pos, double* vel, const float* T,
                   const int64_t* ids, const int64_t* ladder_ids, int64_t B, double to_nm, int32_t* walker,
                   float* out_frames, double* out_epot, double* out_ekin, int32_t* out_walker, int64_t* out_counts, int mem);
/* The log-weights of the TI map from reduced energies: out_logw[b] = -(u1[b] - u0[b] + neg_dlogp[b]) (the reference's weight is
 * exp(-(E1 - E0 + neg_dlogp)), ess.py:8-10), formed in fp64 as ((u1 - u0) + neg_dlogp) and rounded once to the fp32 that
 * ti_obs_weights, ti_obs_hist, ti_obs_bootstrap and ti_obs_rff_gram take.  u0, u1 [B] fp64, neg_dlogp [B] fp32, out_logw [B] fp32:
 * [host|device] by mem.  u0 == NULL: 0 (the calc_phis_bg form); neg_dlogp == NULL: 0.  Non-finite inputs pass through: the
 * consumers refuse them by index.  Any handle.  TI_E_ARG: a NULL handle, u1 or out_logw, B < 1, an unknown mem. */
int ti_obs_ti_logw(ti_handle* h, const double* u0, const double* u1, const float* neg_dlogp, int64_t B, float* out_logw, int mem);
/* The log-weights of a Boltzmann generator, and of a latent -> ambient chain, from the prior samples the run started from (the
 * reference's weight is exp(-E1 - log N(z0; 0, I) - (neg_dlogp_bg + neg_dlogp_ti)), ess.py:13-29 calc_log_mvnormal_pzs and
 * calc_importance_weights).  All in fp64:
 *   out_logpz[b] = -(0.5 * S_b) - (m * TI_BG_HALF_LOG_2PI),   S_b = sum_j (double)z[b][j]^2
 *   out_logw[b]  = -(((u1[b] + out_logpz[b]) + neg_dlogp_bg[b]) + neg_dlogp_ti[b])
 * out_logw rounded once to the fp32 that ti_obs_weights, ti_obs_hist, ti_obs_bootstrap and ti_obs_rff_gram take.  z [B][m] fp32,
 * one row per molecule (a molecule handle: m = 3A; m is an argument, so the d-dimensional toy models can call it too); u1 [B] fp64
 * the reduced energy of the generated state (NULL: 0); neg_dlogp_bg, neg_dlogp_ti [B] fp32 (NULL: 0); out_logpz [B] fp64 and
 * out_logw [B] fp32, either may be NULL but not both.  All [host|device] by mem.  Any handle.
 * One wave per molecule, four molecules per workgroup: lane l adds the squares of components l, l + 64, ... in that order and the
 * 64 lane sums are combined by the fixed butterfly with offsets 32 .. 1; no atomics.  Every term of S_b is exact (the square of an
 * fp32 value fits fp64's mantissa) and m * TI_BG_HALF_LOG_2PI is rounded before the subtraction (no contraction), so a molecule's
 * outputs are a function of its row and m only -- not of B, of the row's place in the batch, of mem or of the launch -- and a numpy
 * restatement reproduces them bit for bit.  Non-finite inputs pass through to that molecule only: the consumers refuse them by
 * index.  TI_E_ARG, nothing written: a NULL handle, z == NULL, both outputs NULL, B < 1, m < 1 or m > TI_BG_MAX_M, an unknown mem. */
#define TI_BG_MAX_M 65536
#define TI_BG_HALF_LOG_2PI 0.9189385332046727
int ti_obs_bg_logw(ti_handle* h, const float* z, int64_t B, int64_t m, const double* u1, const float* neg_dlogp_bg, const float* neg_dlogp_ti,
                   double* out_logpz, float* out_logw, int mem);
/* The effective sample size (sum w)^2 / sum w^2 (the reference's calc_ESS) of the same weights from their UNROUNDED fp64 logarithms
 * l[b] = -(((u1[b] + logpz[b]) + neg_dlogp_bg[b]) + neg_dlogp_ti[b]), logpz [B] fp64 as ti_obs_bg_logw returns it, over the molecules
 * with keep[b] != 0 (keep [B] uint8; NULL: all -- the once-filtered sample of gen_ess_bg).  The one fp32 rounding of out_logw moves an
 * ESS by up to 2e-6 relative; this entry has no such term and agrees with calc_ESS of the reference's fp64 weights to the summation
 * error.  w = exp(l - max l).  One workgroup: thread t walks molecules t, t + 256, ... in that order, the 256 partial results meet in
 * a fixed tree; fp64, no atomics, so a call repeats bit for bit.  Arrays [host|device] by mem; out_ess and out_kept (may be NULL)
 * are host scalars.  Any handle.  TI_E_NAN with the index for a non-finite kept l; TI_E_ARG: NULL logpz or out_ess, an unknown mem,
 * B < 1, a NULL handle, a keep that leaves no molecule. */
int ti_obs_bg_ess(ti_handle* h, const double* logpz, int64_t B, const double* u1, const float* neg_dlogp_bg, const float* neg_dlogp_ti,
                  const uint8_t* keep, double* out_ess, int64_t* out_kept, int mem);
/* ---- Z-matrix (internal) coordinates: construct, NeRF rebuild with log|det J|, and the histograms of all columns ------------------
 * What the reference's mdqm9/analysis/utils/z_matrix.py computes around results_00031.py: construct_z_matrix_batch on the sorted
 * atoms (ti_obs_zmat), deconstruct_z_matrix_batch -- the batch version, which does not clamp --, its log-determinant
 * (jacobian=True, compute_jacobian_batch) and the validity screen correct_conf_indexes (ti_obs_zmat_xyz).  fp64 arithmetic on the
 * fp32 inputs, no atomics; a molecule's outputs are a function of its own inputs and the topology only -- not of its place in the
 * batch, of B or of mem -- and a call repeats bit for bit.
 * Topology (host memory, copied per call like desc of ti_obs_cv): order [A] int32 is a permutation, sorted atom s is the caller's
 * atom order[s] (the reference's atom_order; NULL: the identity); ref [A][3] int32 in SORTED numbering (the reference's ref_atoms):
 * ref[s] = (r1, r2, r3) gives sorted atom s the distance DIST(s, r1), the angle ANGLE(s, r1, r2) at r1 and the torsion
 * TORSION(r3, r2, r1, s) of ti_obs_cv -- compute_distance(x4, x3), compute_angle(x4, x3, x2), compute_torsion(x1, x2, x3, x4) of
 * z_matrix.py:86-93.  Only ref[s][0] is read for s >= 1, ref[s][1] for s >= 2 and ref[s][2] for s >= 3; the slots read must be < s
 * and distinct.
 * Both calls take painn handles with 2 <= A <= 32 (an adw handle: TI_E_ARG); with ti_painn_set_molecules in force they return
 * TI_E_UNSUPPORTED: one topology is one species.  TI_E_ARG, before any device work and with nothing written: order not a
 * permutation, a slot that is read outside 0..s-1 or repeated, ref == NULL, B < 0, a NULL x / z or output with B > 0, an unknown
 * mem.  B = 0: TI_OK.
 *
 * ti_obs_zmat: x [B,A,3] fp32 -> out_z [B,A-1,3] fp32, both [host|device] by mem.  Row s - 1 is (d, a, t) of sorted atom s; a = 0
 * in row 0 and t = 0 in rows 0 and 1, exactly (the reference's layout).  One thread per (molecule, row); every value holds the bits
 * ti_obs_cv returns for the equivalent descriptor on the caller's atoms (the angle is atan2(|u x v|, u.v), not the reference's fp32
 * acos). */
int ti_obs_zmat(ti_handle* h, const int32_t* order, const int32_t* ref, const float* x, int64_t B, float* out_z, int mem);
/* ti_obs_zmat_xyz: z [B,A-1,3] fp32 -> out_x [B,A,3] fp32 in the caller's atom numbering, in the reference's canonical frame; with
 * (d, a, t) = row s - 1 of z as fp64 and X the placed fp64 positions:
 *   sorted atom 0 at the origin, sorted atom 1 at (z[0,0], 0, 0),
 *   sorted atom 2 at (X[ref[2][0]].x - d cos a, d sin a, 0) if ref[2][0] != 0, else at (d cos a, d sin a, 0),
 *   sorted atom s >= 3 with p3 = X[r1], p2 = X[r2], p1 = X[r3]: e1 = (p3 - p2) / |p3 - p2|, n = (p2 - p1) x e1 / |.|, e2 = n x e1,
 *   X[s] = p3 - d cos a e1 + d sin a cos t e2 + d sin a sin t n
 * -- ic_to_xyz of mol_geometry.py with cos(pi - a) = -cos a and sin(pi - a) = sin a, so that no rounded pi enters.  Positions are
 * rounded to fp32 once, on output.  The structural zeros of z are not read except by out_valid.
 * out_logdet [B] fp64 (may be NULL): log|z[1,0]| + sum over s >= 3 in ascending s of (2 log|z[s-1,0]| + log|sin z[s-1,1]|), 0 for
 * A = 2: the closed form of the reference's det J_2 and det J_det (log|det| of the map from the 3A - 6 internal coordinates).
 * out_valid [B] uint8 (may be NULL): correct_conf_indexes as a mask, 1 iff every one of the A - 1 rows has d > 0, 0 <= a <= pi32 and
 * -pi32 < t <= pi32, compared in fp32 with pi32 = (float)pi, the structural zeros included as they are given; a NaN gives 0.
 * out_x, out_logdet, out_valid: [host|device] by mem.
 * One thread per molecule (the chain is sequential), 64 molecules per workgroup, the placed positions in LDS (1536 A bytes).
 * Degenerate input is not an error: collinear references, d = 0 or sin a = 0 give NaN or +-inf in that molecule's outputs only. */
int ti_obs_zmat_xyz(ti_handle* h, const int32_t* order, const int32_t* ref, const float* z, int64_t B, float* out_x, double* out_logdet,
                    uint8_t* out_valid, int mem);
/* ti_obs_hist for every column of values [B,K] fp32 in one launch: column c is binned into n_bins equal bins on [lo[c], hi[c])
 * (lo, hi [K] fp64, host) by the rules of ti_obs_hist -- a value equal to hi[c] is in the upper tail --, 1 <= n_bins <= 256,
 * 1 <= K <= 128; out_hist [K][n_bins] and out_tails [K][3] (host, double).  The sums of a column are taken in the order ti_obs_hist
 * takes them: with keep == NULL column c holds the bits of ti_obs_hist(values + c, stride K, ...).
 * keep [B] uint8 (may be NULL; [host|device] by mem like values and logw): entries with keep[i] == 0 get weight 0, and the max
 * shift, the normalising sum and the refusal of a non-finite logw run over the kept entries only (logw == NULL: 1 / #kept), so the
 * kept weights sum to 1.  Any handle.  TI_E_ARG: n_bins, K or a range as above, B < 1, a NULL buffer, an unknown mem, a keep that
 * keeps nothing; TI_E_NAN: a non-finite kept logw (the message names the first such index). */
int ti_obs_hist_cols(ti_handle* h, const float* values, int32_t K, const float* logw, const uint8_t* keep, int64_t B, int32_t n_bins,
                     const double* lo, const double* hi, double* out_hist, double* out_tails, int mem);
/* Time-lagged independent component analysis (TICA) of featurised trajectories: what the reference's mdqm9/plots/10506_main.ipynb
 * (cell 3) does with deeptime.decomposition.TICA(lagtime, dim) on the (cos, sin) encoding of the torsions.  The estimator is
 * defined here, after deeptime's documented reversible one; parity with deeptime's own numbers is not pinned.
 * Inputs.  values fp32: feature column k of frame i is values[i * stride + k * cstride], cstride >= 1, stride >= (K - 1) cstride + 1
 * (the torsion column of a [B, A-1, 3] Z-matrix array is read in place: base offset 8, cstride 3, stride 3 (A - 1)); 1 <= K <=
 * TI_TICA_MAX_K.  encode = 1: d = 2 K, feature 2k = cos x_k, 2k + 1 = sin x_k (fp64 sincos of the fp32 value); encode = 0: d = K, the
 * value itself.  d <= TI_EIGH_MAX_N.  traj_off [n_traj + 1] int64, host: strictly ascending, traj_off[0] = 0, traj_off[n_traj] = n;
 * frames traj_off[t] .. traj_off[t + 1] - 1 are trajectory t in time order (ragged trajectories are allowed).  lags [n_lag] int32,
 * host, each >= 1, 1 <= n_lag <= TI_TICA_MAX_LAGS.
 * Pairs.  The pairs of lag tau are (i, i + tau) with both frames in one trajectory, ordered trajectory-major, then i ascending;
 * N_tau their count.  A trajectory of length <= tau contributes none.  N_tau < 2 is refused.
 * Moments.  With X the first and Y the second frames of the pairs: sx = sum X, sy = sum Y, Sxx = X^T X, Syy = Y^T Y, Sxy = X^T Y, fp64.
 * ti_obs_tica_moments: count [n_lag] int64 = N_tau, sum [n_lag, 2, d] = (sx, sy), cov [n_lag, 3, d, d] = (Sxx, Syy, Sxy).  A feature
 * pass writes an fp64 table [n][D] once per call, D = d rounded up to 16: n D > 2^27 is TI_E_ALLOC.  One 256-thread workgroup per
 * (lag, segment of 8192 pairs) contracts on v_mfma_f64_16x16x4_f64, four pairs per step, the two table rows of 16 pairs at a time
 * staged through LDS (upper-triangle 16 x 16 tiles of Sxx and Syy, all tiles of Sxy; the column sums as one more product).  Every
 * tile and every sum runs over a segment's pairs in pair order, the segments are added in order by a second kernel, Sxx and Syy are
 * mirrored and exactly symmetric, and there are no atomics: a lag's result is a function of (the data, traj_off, tau) only -- not
 * of the other lags of the call, of mem, or of how the lags share launches -- and a call repeats bit for bit.
 * TI_E_ARG, before any device work: a NULL handle or buffer; an unknown mem; K, d, n_lag, n, n_traj or the strides out of range; encode
 * not 0 or 1; a lag < 1; a traj_off that is not as above; N_tau < 2 (the lag is named).  TI_E_NAN, nothing written: a non-finite
 * value (found on the device; the first such row is named).
 * Model (ti_obs_tica_fit), per lag, with N = N_tau: mu = (sx + sy) / (2 N), C00 = (Sxx + Syy) / (2 N) - mu mu^T, C0t = (Sxy + Sxy^T) /
 * (2 N) - mu mu^T.  The eigenpairs (s, V) of C00 in descending order, r = #{s_k > epsilon} (epsilon absolute), L = V[:, :r] /
 * sqrt(s[:r]), Kt = L^T C0t L of which the upper triangle is read, its eigenpairs (lambda, U) in descending order, R = L U[:, :dim].
 * In each column of R the entry of largest magnitude is made positive (among exactly equal magnitudes the lowest feature index
 * decides); scaling = 1 ("kinetic map") then multiplies column k by lambda_k, scaling = 0 leaves it.  Columns and eigenvalues at index
 * >= r are NaN; rank = r is returned and that is not an error.  Both solves are ti_obs_eigh's Jacobi kernel on the real symmetric
 * matrix as a Hermitian one with zero imaginary part: its order, its tie rule, its TI_E_UNSUPPORTED after 64 sweeps.  Around them
 * run fixed-order fp64 kernels, one workgroup per lag.  Results reach the outputs only when the whole call succeeded.
 * TI_E_ARG, before any device work: a NULL handle or buffer, an unknown mem, n_lag or d out of range, dim outside 1..d, a non-finite
 * or negative epsilon, scaling not 0 or 1, reserved not 0; then a count < 2.  TI_E_NAN: a non-finite moment.
 * Projection (ti_obs_tica_transform), all lags in one launch: y_k = sum_f (phi_f(x) - mu_f) R_fk in fp64, f ascending, rounded once
 * to fp32; a non-finite value in a row gives NaN in that row's outputs; a row's output is a function of the row and the model
 * alone.  TI_E_ARG: a NULL handle or buffer, an unknown mem, B < 1, K, d (which must be K or 2 K by encode), dim, n_lag or the
 * strides out of range. */
#define TI_TICA_MAX_LAGS 32
#define TI_TICA_MAX_K 32
typedef struct { int32_t dim, scaling, reserved; double epsilon; } ti_tica_desc;   /* 24 bytes, reserved = 0 */
/* values fp32, count int64, sum, cov fp64: [host|device] by mem; traj_off int64 and lags int32: host */
int ti_obs_tica_moments(ti_handle* h, const float* values, int64_t stride, int64_t cstride, int64_t n, int32_t K, int32_t encode,
                        const int64_t* traj_off, int64_t n_traj, const int32_t* lags, int32_t n_lag, int64_t* count, double* sum, double* cov,
                        int mem);
/* count, sum, cov as ti_obs_tica_moments writes them; mean [n_lag, d], ev [n_lag, dim], comp [n_lag, d, dim] fp64, rank [n_lag] int32:
   [host|device] by mem */
int ti_obs_tica_fit(ti_handle* h, const int64_t* count, const double* sum, const double* cov, int32_t n_lag, int32_t d, const ti_tica_desc* desc,
                    double* mean, double* ev, double* comp, int32_t* rank, int mem);
/* values fp32 (B rows), mean, comp fp64, out [n_lag, B, dim] fp32: [host|device] by mem */
int ti_obs_tica_transform(ti_handle* h, const float* values, int64_t stride, int64_t cstride, int64_t B, int32_t K, int32_t encode,
                          const double* mean, const double* comp, int32_t n_lag, int32_t d, int32_t dim, float* out, int mem);
/* Observer: with one attached, every rollout entry point (ti_painn_rollout, _dlogp, _dlogp_est, ti_adw_rollout, _dlogp) also
 * evaluates the K CVs on the state at the grid points i with i % every == 0 and at the last one -- ti_rollout_rows(n_step, every)
 * rows, whatever save_every is -- and writes them to out_cv [rows, B, K] fp32 ([host|device] by mem; the caller sizes it for the
 * rollouts that follow and keeps it alive).  Where a path row is written at the same grid point, the CVs are those of exactly
 * that row (dopri5: of the dense output evaluated there).  desc, ref and select as in ti_obs_cv, copied into the handle; every >= 0
 * (0: the last grid point only).  desc == NULL detaches.  Path, dlogp and n_fevals of a rollout do not depend on the observer, and
 * without one a rollout takes exactly the launches it took before.  TI_SCHEME_DOPRI5_TRAJ writes its rows per trajectory inside a
 * kernel: with an observer attached it returns TI_E_UNSUPPORTED. */
int ti_obs_set_observer(ti_handle* h, const int32_t* desc, int32_t K, const float* ref, const int32_t* select, int32_t every,
                        float* out_cv, int mem);
/* Pre-size the HBM workspace for batches up to B trajectories (otherwise grown on demand). */
int ti_reserve(ti_handle* h, int64_t B);
/* Live kernel timing with HIP events on the handle's stream (bench.py roofline leg). */
enum { TI_KERNEL_PAINN_EDGE = 0, TI_KERNEL_PAINN_UPDATE = 1, TI_KERNEL_PAINN_EMBED = 2, TI_KERNEL_PAINN_READOUT = 3,
       TI_KERNEL_ADW = 4, TI_KERNEL_INTEGRATE = 5, TI_KERNEL_PAINN_JVP_EDGE = 6, TI_KERNEL_PAINN_JVP_UPDATE = 7,
       TI_KERNEL_PAINN_JVP_READOUT = 8, TI_KERNEL_PAINN_JVP_FILTER = 9, TI_KERNEL_COUNT = 10 };
int ti_profile_enable(ti_handle* h, int on);
int ti_profile_read(ti_handle* h, int kernel, int64_t* n_launches, double* total_ms);   /* also resets that slot */
/* Debug taps for parity tests: copy an intermediate of the LAST ti_painn_drift / ti_painn_drift_jvp call to host.
 * what: 0 = s [B,A,F], 1 = v [B,A,3,F] (component-major planes), 2 = e (row-major [B,E_m,F], edges in (dst,src) order);
 * 3, 4, 5 = the tangents of s, v, e of the last ti_painn_drift_jvp call, same shapes. */
int ti_painn_debug_tap(ti_handle* h, int stop_after_stage);   /* stage = 0 embed, 1+2l message l, 2+2l update l; -1 = off */
int ti_painn_debug_read(ti_handle* h, int what, float* out, size_t n_floats);
/* Test hook for the first-touch accumulators (csrc/painn_edge_kernel.hpp: acc_out): fill the per-atom accumulators dsacc / dvacc / cacc of
 * the workspace for B trajectories with `value` (NaN, 1e30 ...) on the handle's stream.  A following ti_painn_drift must return exactly what
 * a handle created with TI_ZERO_ACC=1 in the environment (zeroing path: memsets + adds only) returns.  Reference counterpart: none
 * (torch_scatter allocates its output, cpainn.py:303-304).  The edge state e and the parked edge geometry (encoding, edge_dir) are filled
 * as well: an evaluation writes every row of them before it reads it, and the pair-major kernel never touches rows of absent pairs. */
int ti_painn_debug_poison(ti_handle* h, int64_t B, float value);
/* Layer-0 phi table.  Entering the first message layer the phi branch sees only the embedding's output and
 * edge_emb[type]: a function of (atom, that molecule's cond rows, t, edge type).  Molecules of a call whose A x ncond cond values are
 * bitwise equal form a class; with at most TI_PHI0_MAX_CLASSES classes the branch is evaluated once per (class, atom, type) into a
 * table and the pair-major message kernel of layer 0 reads it, bit for bit the value it would have computed.  More classes, per-molecule
 * times, tangent passes, an edge mask / mixed species, a debug tap, precisions other than f16x2, the directed layouts, or
 * TI_PHI0_TABLE=0 in the environment when the handle is created: the kernels of before run unchanged. */
#define TI_PHI0_MAX_CLASSES 16
/* which path layer 0 of the LAST drift evaluation of the handle took (a rollout: its last evaluation): 1 = table, 0 = fallback,
 * -1 = no evaluation yet.  *n_classes (may be NULL): classes found by the call's class pass (TI_PHI0_MAX_CLASSES + 1: more than the
 * cap), 0 when the call ran none. */
int ti_painn_debug_phi0_path(ti_handle* h, int32_t* n_classes);
/* The pair-major template of the handle: molecules per group, row blocks per group, and how many of them -- the
 * leading ones -- are 4 x 4 tiles; the rest are general blocks of 16 unrelated pairs (n_tile == nblk: none, e.g. with TI_PAIR_PACKED=0
 * in the environment when the handle was created).  Returns 1, or 0 when the handle has no pair template (nothing is written). */
int ti_painn_debug_pair_blocks(ti_handle* h, int32_t* G, int32_t* nblk, int32_t* n_tile);
/* Seeded accumulators.  A packed pair template is seeded when its general rows name every atom of every molecule of a
 * group exactly once (the complete graph on 18 atoms: the 36 twin pairs of 4 molecules).  The message layers of an evaluation in the
 * pair layout then launch the general blocks FIRST -- each row stores its two contributions, every atom's first of the layer, no
 * atomic and no read -- and the tile blocks after them, which only add.  Every other evaluation keeps the order of before (tiles whose
 * first touch replaces the accumulator, then general rows that add): f32 handles, an edge mask or mixed species in force (a mask that
 * removes no edge of any molecule leaves the template's rows as they are and counts as none here), the directed layouts, a template
 * that is not seeded, or TI_PAIR_SEEDED=0 in the environment when the handle is created.
 * Returns which order the LAST drift evaluation of the handle took (a rollout: its last evaluation): 1 = seeded, 0 = the order of
 * before, -1 = no evaluation yet.  *template_seeded (may be NULL): 1 when the handle's pair template is seeded, else 0. */
int ti_painn_debug_pair_seeded(ti_handle* h, int32_t* template_seeded);
/* Merged tails.  The last general block of a seeded template may hold r < 16 valid rows (18 atoms at G = 4: 36 twin
 * pairs = 16 + 16 + 4).  Where r is a multiple of 4 that divides 16, the seeded general launch gives one wave S = 16 / r groups: it
 * walks their full general blocks, then their S last blocks as ONE block of 16 rows.  Storage, row words and results are those of the
 * walk of one group per wave, bit for bit.  TI_PAIR_TAILS=0 in the environment when the handle is created keeps that walk.
 * Returns which walk the general launches of the LAST drift evaluation took: 1 = merged tails, 0 = one group per wave (or no seeded
 * launch at all), -1 = no evaluation yet.  *groups_per_wave (may be NULL): S of the handle's pair template, 0 when it has no such tails. */
int ti_painn_debug_pair_tails(ti_handle* h, int32_t* groups_per_wave);
/* Embed per class.  On the phi table path the embedding is read twice: P of the class representatives by the table
 * kernel, s once by layer 0's update kernel; the embed rows of a class's molecules agree bit for bit.  The embed launch of such an
 * evaluation then covers the (class, atom) rows alone, the table kernel reads them, and layer 0's update kernel reads s through the
 * class map and is the first to write the full s and P: bit for bit the result of the launch over every atom.  Every evaluation off
 * the table path, or TI_EMBED_CLASSES=0 in the environment when the handle is created: the embed launch of before.
 * Returns which embed launch the LAST drift evaluation of the handle ran (a rollout: its last evaluation): 1 = per class, 0 = every
 * atom, -1 = no evaluation yet.  ti_painn_debug_poison fills the full s and P as well, which such an evaluation must not read. */
int ti_painn_debug_embed_path(ti_handle* h);
/* Update launches that keep v_eff in registers.  The update kernel forms v_eff = v + dv in its first phase and needs it
 * again in its last; the builds of before park it in the dv accumulator in between.  The f16x2 builds up to F = 128 have twins that
 * keep components of it in fp32 registers instead -- the same values in the same expressions, bit for bit the results of before --
 * and a handle launches those unless TI_UPDATE_KEEP=0 is in the environment when it is created.
 * Returns how many of the three components the update launches of the LAST drift evaluation kept: 1..3, 0 = the builds of before (the
 * switch, f32, the fp16 storage mode, F = 256), -1 = no evaluation yet. */
int ti_painn_debug_update_keep(ti_handle* h);
/* Device self-test of the MFMA operand/accumulator lane maps the kernels rely on, of both fp32 -> (hi, lo) fp16 operand splits
 * (the 8-instruction forms of formats (a) and (b) against the plain arithmetic, bit for bit, fp16-subnormal residuals included),
 * and of the fp16 matrix instruction keeping subnormal inputs. */
int ti_selftest(int device);

/* ---- velocity loss: the stochastic-interpolant objective a checkpoint was trained on, forward evaluation only ---------------------
 * The reference's model-quality number (mdqm9/thermo/{ambient,latent}/losses.py, adw/thermo/losses.py with the interpolants.py beside
 * them; evaluated on held-out pairs by train_ambient.py:153-157): antithetic states from an interpolant, the drift on both, and a
 * per-molecule sum.  Three stages on the handle's stream, no atomics, every sum in an order fixed by the shapes alone, so a call
 * repeats bit for bit.  State rows: a molecule's [A,3] coordinates (painn, m = 3A) or a particle's [d] (adw, m = d).
 *
 * Interpolate (fp64 from the fp32 inputs, one rounding to fp32).  With t_b the time of molecule / row b and z the noise:
 *   TI_VLOSS_STANDARD   xt+- = (1 - t) x0 + t x1 +- gamma(t) z             (LinearInterpolant.calc_antithetic_xts)
 *   TI_VLOSS_ONE_SIDED  xt+  = t x1 + (1 - t) x0, x0 being the noise itself  (OneSidedLinearInterpolant; the reference computes the
 *                       minus state and discards it: it is neither written nor evaluated here, and z must be NULL)
 *   gamma kinds (parameter a):  TI_GAMMA_BROWNIAN  gamma = sqrt(a t (1 - t)),  gamma' = a (1 - 2t) / (2 sqrt(a t (1 - t)))
 *                               TI_GAMMA_SIN2      gamma = sin^2(pi t),        gamma' = 2 pi sin(pi t) cos(pi t)
 *                               TI_GAMMA_SIG_SUM   gamma = 2.2 (s(u+) - s(u-) - s(1 - a/2) + s(-1 - a/2)),
 *                                                  gamma' = 2.2 a ((1 - s(u+)) s(u+) - (1 - s(u-)) s(u-)),  u+- = a (t - 1/2) +- 1,
 *                                                  s the logistic function; 2.2 is the float32 nearest to it, which is what the
 *                                                  reference multiplies by (torch.tensor(2.2)).  The reference holds a as a float32
 *                                                  tensor too: a is used as passed, so pass (double)(float)a to reproduce it (the
 *                                                  Python mirror does)
 *   centring:  TI_CENTER_BATCH     the reference's xt - mean(xt, dim=0): the mean over all B A atom rows of the CALL, per component,
 *                                  separately for the plus and the minus half (so the result depends on how a set is cut into calls);
 *                                  the column sums are taken over fixed tiles of 1024 rows and then over the tile sums, in the fixed
 *                                  order stated under Reduce
 *              TI_CENTER_MOLECULE  each molecule's own centre (atoms summed in order): independent of the other molecules
 *              TI_CENTER_NONE      the only mode of an adw handle
 *   z == NULL:  z[b,a,c] = N(seed, traj_offset + b, draw, 3a + c) (adw: component k), N the Philox normal of TI_SCHEME_EM with `draw`
 *               in its step slot, AS THE HOST ORACLE RETURNS IT: oracle.normal regenerates every entry bit for bit.  The counter
 *               slots and the fp32 Box-Muller expression are those of the EM noise; its logf, sinf and cosf are evaluated here by
 *               the host libm's own algorithms restated in fp64 (glibc's since 2.28, which are the Arm Optimized Routines':
 *               csrc/vloss_normal.hpp), where the EM noise kernels call the device's fp32 functions and agree with the oracle to the
 *               last bits only.  The identity is therefore tied to that libm: an oracle built against another logf / sinf / cosf
 *               may differ from z in the last bit.
 *   t:  TI_TDIST_GIVEN  t [B] as passed (t == NULL otherwise).  Drawn times take ONE word per molecule,
 *         o = Philox4x32-10(counter = (id & 0xffffffff, id >> 32, draw, TI_VLOSS_DOMAIN), key = (seed & 0xffffffff, seed >> 32)),
 *         id = traj_offset + b,  u = ((o[0] >> 9) + 0.5) 2^-23 -- exact in fp32 and never 0 or 1 -- and
 *         TI_TDIST_UNIFORM   t = u                                           (torch.rand)
 *         TI_TDIST_BETA_HALF t = fp32(sin^2(pi u / 2)) in fp64               (Beta(1/2, 1/2), ambient t_distr = "beta")
 *         TI_TDIST_BETA_2_1  t = fp32(sqrt(u)) in fp64                       (Beta(2, 1), latent t_distr = "beta")
 *         each capped at 1 - 2^-24, the largest fp32 below 1, so that 0 < t < 1 always.
 *       These draws follow the reference's DISTRIBUTIONS; they do not reproduce torch's random streams (neither for t nor for z).
 * Drift.  One evaluation of the per-molecule-time drift (ti_painn_drift_tv / ti_adw_drift_tv) on the device-resident batch
 *   [xt+; xt-] of 2B (one-sided: xt+, B) with times [t; t] and conditioning [cond; cond].  As for the drift itself, the layout
 *   follows the evaluated batch size unless it is pinned (ti_painn_set_template).  In a layout that packs G > 1 molecules into a row
 *   group a molecule's per-atom sums follow its slot in the group, so the batch is laid out with molecule b of either half at slot
 *   (traj_offset + b) mod G -- up to G - 1 copies of the call's first molecule in front of each half, their results dropped; the
 *   halves are written where they belong, so no pass over the states is added.  (The padded count is what the layout is chosen
 *   from; should that choice not settle on one G within eight rounds, the batch is evaluated unaligned.)  With the
 *   layout pinned and traj_offset the global index of molecule 0, l_b under TI_CENTER_MOLECULE and TI_CENTER_NONE is then the same
 *   bits however a set is cut into calls (t and z always are); an adw row never depends on the others.  An edge mask in force (for B
 *   molecules) applies to both halves, which are then evaluated one after the other as two batches of B, without that alignment.
 * Reduce (fp64, element order).  With d = x1 - x0 and the sum over the m entries of a row:
 *   STANDARD   l_b = sum [ b+^2 / 2 - (d + gamma' z) b+ + b-^2 / 2 - (d - gamma' z) b- ]        ONE_SIDED   l_b = sum [ b+^2 / 2 - d b+ ]
 *   Every product, sum and difference of l_b is rounded on its own (no fused multiply-add), the four terms of an entry added in the
 *   order written: with BROWNIAN, l_b is the plain IEEE double evaluation of this expression from t, z and b.
 *   *out_mean = sum_b l_b / (B A) for molecules (the reference's mean over atom rows) and / B for adw.  Every batch-wide sum (this
 *   one, the column sums of TI_CENTER_BATCH, the time profile) is taken by 256 accumulators that start at +0.0 and are then folded
 *   by one fixed tree: for s = 128, 64, .., 1, accumulator i < s takes accumulator i + s.  Within a tile of 1024 values accumulator
 *   j adds values 4j .. 4j + 3 of the tile in order; across the tiles accumulator j adds the sums of tiles j, j + 256, .. in order.
 *   out_tbins [n_tbins][2]: sum of l_b and count of the molecules with floor(t_b n_tbins) = k (t = 1 in the last bin); per bin,
 *   accumulator j adds the matching molecules among j, j + 256, .. in order (no tiles).  None of these is a plain sequential sum,
 *   and none depends on anything but the values and their number: not on the launch, the device or the memory space.
 * Buffers.  x0, x1 [B,m], cond (painn) / beta0, beta1 [B] (adw), t [B], z [B,m], out_t [B], out_z [B,m], out_xt, out_b [2,B,m]
 *   (plus, then minus; ONE_SIDED writes the first half only) fp32 and out_loss [B] fp64: [host|device] by mem.  out_mean [1] and
 *   out_tbins [n_tbins,2] fp64: host.  Every out_* but out_loss may be NULL; out_t / out_z return what the kernels used (out_z with
 *   ONE_SIDED: nothing is written).  Outputs are copied from buffers of the handle after the whole call succeeded.
 * TI_E_ARG, before any device work, in this order: a NULL descriptor; an unknown kind, gamma, center or t_dist; a <= 0 or not finite
 *   where gamma uses it (STANDARD with BROWNIAN or SIG_SUM); n_tbins outside 0..TI_VLOSS_MAX_TBINS; B < 1; an unknown mem; ONE_SIDED
 *   with a non-NULL z; t_dist GIVEN without t, or t with another t_dist; a given t in host memory outside [0, 1] or not finite, or equal
 *   to 0 or 1 with STANDARD and BROWNIAN (gamma' is infinite there); a NULL buffer; a NULL or wrong-kind handle.
 * TI_E_UNSUPPORTED: ti_painn_set_molecules in force (one species per call, as for ti_obs_ff_energy); BATCH or MOLECULE on an adw handle.
 * TI_E_NAN: a non-finite l_b, naming the first such molecule (e.g. a given t in device memory at 0 with BROWNIAN, which is not read on
 *   the host); no output is copied. */
enum { TI_VLOSS_STANDARD = 0, TI_VLOSS_ONE_SIDED = 1 };
enum { TI_GAMMA_BROWNIAN = 0, TI_GAMMA_SIN2 = 1, TI_GAMMA_SIG_SUM = 2 };
enum { TI_CENTER_BATCH = 0, TI_CENTER_MOLECULE = 1, TI_CENTER_NONE = 2 };
enum { TI_TDIST_GIVEN = 0, TI_TDIST_UNIFORM = 1, TI_TDIST_BETA_HALF = 2, TI_TDIST_BETA_2_1 = 3 };
#define TI_VLOSS_DOMAIN 0x564c4f53u   /* the fourth counter word of the time draws ("VLOS") */
#define TI_VLOSS_MAX_TBINS 1024
typedef struct ti_vloss_desc {
    int32_t  kind;         /* TI_VLOSS_* */
    int32_t  gamma;        /* TI_GAMMA_*; ignored by ONE_SIDED */
    double   a;            /* gamma's parameter */
    int32_t  center;       /* TI_CENTER_* */
    int32_t  t_dist;       /* TI_TDIST_* */
    uint64_t seed;         /* Philox key of the drawn t and z */
    int64_t  traj_offset;  /* global index of molecule 0 of this call: the draws do not depend on how a set is cut into calls */
    int32_t  draw;         /* the draw index (the step slot of the counter) */
    int32_t  n_tbins;      /* bins of the time profile; 0: none */
} ti_vloss_desc;
int ti_painn_vloss(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* cond, const float* t,
                   const float* z, int64_t B, double* out_loss, double* out_mean, double* out_tbins, float* out_t, float* out_z,
                   float* out_xt, float* out_b, int mem);
int ti_adw_vloss(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* beta0, const float* beta1,
                 const float* t, const float* z, int64_t B, double* out_loss, double* out_mean, double* out_tbins, float* out_t,
                 float* out_z, float* out_xt, float* out_b, int mem);
/* stage one alone: out_xt [2,B,m] is required, out_t and out_z may be NULL; same checks */
int ti_painn_vloss_interp(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* t, const float* z,
                          int64_t B, float* out_t, float* out_z, float* out_xt, int mem);
int ti_adw_vloss_interp(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* t, const float* z,
                        int64_t B, float* out_t, float* out_z, float* out_xt, int mem);

/* ---- adw trainer: FCNetMultiBeta trained on the velocity loss, on the device --------------------------------------------------------
 * The training stage of the adw workflow (adw/train.py: StandardVelocityLoss / OneSidedVelocityLoss on FCNetMultiBeta(d, d, H, L),
 * torch.nn.utils.clip_grad_norm_, torch.optim.Adam with L2 weight decay, the NaN skip of its lines 59-65).  A trainer is a handle of
 * its own kind, freed by ti_destroy.  It owns, in device memory: the master weights and the Adam moments m, v in fp64 (the reference
 * trains in float64; fp32 masters would lose the late, small-learning-rate updates), and an fp32 working copy of the weights in the
 * canonical layout of ti_adw_create_nd, refreshed by the optimiser kernel.  A drift handle stays immutable: every painn / adw entry
 * point refuses a trainer handle with TI_E_ARG ("not an adw handle"), and the calls below refuse any other handle the same way.
 * ti_adw_trainer_create takes the descriptor, dim and weights of ti_adw_create_nd with the same checks in the same order, then:
 * TI_PREC_F16X2 is TI_E_UNSUPPORTED (the trainer takes TI_PREC_F32 only); a NULL train descriptor, lr <= 0, beta1 or beta2 outside
 * [0, 1), eps <= 0, weight_decay < 0 (or any of them not finite) are TI_E_ARG.  All before any device call.
 *
 * Loss.  The states, the drawn t and z, the loss rows l_b and *out_mean = sum_b l_b / B are the velocity-loss block's above, by the
 *   same kernels (interpolate, reduce, the fixed tree), on the drift the trainer's own forward pass gives.  That pass keeps every
 *   layer's activation and is a different kernel from the drift's: each pre-activation is one fmaf chain over the layer's inputs in
 *   order from +0.0, the bias added afterwards.  Its relation to ti_adw_vloss on an f32 drift handle of the same weights is
 *   therefore closeness (fp32 round-off), not identity.
 * Backward.  The gradient is of the MEAN loss: d / d b+- = (b+- - target+-) / B with target+- = (x1 - x0) +- gamma'(t) z, computed
 *   in fp64 and rounded to fp32 once; ONE_SIDED has the plus half only.  Backward through net runs on the 2B rows [xt+; xt-]
 *   (ONE_SIDED: B).  beta_embed is evaluated once per row b -- (beta0, beta1, t) is shared by the halves -- and receives the
 *   gradient of net.0's embedding input column of both halves: sum_n W0[n][d+1] (g+_bn + g-_bn), the halves added in that order,
 *   n in order, in fp64 from the fp32 g and rounded to fp32 once (the halves are antithetic and the sum cancels).  silu'(z) = s +
 *   silu(z) (1 - s), s the logistic function, as in the tangent code of the drift.  All matrix products run on
 *   v_mfma_f32_16x16x4_f32, each output element one fmaf chain in index order.  The weight gradient contracts over the rows in
 *   slices of 512 rows (row order within a slice); the slice results (fp32) are added in fp64 in slice order from +0.0.  A bias
 *   gradient is the column sum of the layer's g over the rows in fp64: accumulator p of 16 adds rows p, p + 16, .. in order from
 *   +0.0, then the accumulators are added in order.  No atomics: a gradient is a function of the weights and the batch --
 *   including the ORDER of its rows -- and not of the launch, the memory space of the inputs, or what ran before.
 * Clipping (clip_grad_norm_).  norm = sqrt(sum g^2) over all parameters in fp64, the sum by the fixed tree of the velocity-loss
 *   block over tiles of 1024 entries in canonical order; coef = min(1, max_grad_norm / (norm + 1e-6)); g <- coef g.  max_grad_norm
 *   <= 0 or inf: no clipping.  Then g <- g + weight_decay p (torch adds the decay inside Adam.step, after the clip; skipped when
 *   weight_decay == 0).
 * Adam.  With k = n_applied + 1:  m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) (g g);
 *   p <- p - (lr / (1 - beta1^k)) (m / (sqrt(v) / sqrt(1 - beta2^k) + eps)).  fp64, every product, sum, quotient and root rounded on
 *   its own; lr / (1 - beta1^k) and sqrt(1 - beta2^k) are computed on the host (pow of the C library) and passed to the kernel.
 * NaN skip.  If the step's mean loss or sum g^2 is not finite (any non-finite gradient entry makes it so), nothing changes: not the
 *   weights, not the moments, not n_applied.  n_skipped is incremented, the step's out_loss entry is NaN, and the following steps
 *   go on.  Decided by the optimiser kernel from the two sums in device memory, without a host synchronisation.
 * ti_adw_train_grad: loss rows, their mean, the gradient of the mean loss at the current weights and its norm; nothing is updated.
 *   out_loss [B] fp64 [host|device] by mem; out_mean, out_grad [n_weights] (canonical layout), out_gnorm fp64 host; any may be NULL.
 *   Non-finite values are returned as they are.
 * ti_adw_train_apply: clip + Adam with a GIVEN gradient (host, fp64, canonical layout); *out_skipped = 1 where a non-finite entry
 *   made the step a skipped one.
 * ti_adw_train_steps: n_steps optimiser steps enqueued on the handle's stream, one synchronisation at the end.  x0 [n0,d], beta0 [n0],
 *   x1 [n1,d], beta1 [n1] are the resident sets; step k uses rows idx0[kB .. kB+B-1] of x0 / beta0 and idx1[..] of x1 / beta1 (int64,
 *   same mem as the data), gathered on the device.  idx0 == idx1 == NULL: n_steps must be 1 and the step uses rows 0..B-1.  (t, z) of
 *   step k: as ti_adw_vloss draws them with draw = desc->draw + k and id = desc->traj_offset + row in the minibatch; TI_TDIST_GIVEN
 *   and a given z only with n_steps == 1.  out_loss [n_steps] fp64 host: the mean loss of every step, NaN where skipped;
 *   *out_skipped: the steps of this call that were skipped.  A skipped step consumes its draw index.
 *   ti_adw_train_steps with n_steps = 1 is ti_adw_train_grad followed by ti_adw_train_apply of its out_grad, bit for bit.
 * ti_adw_train_get_state / set_state: master weights and moments [n_weights] fp64 host (NULL: not copied / left as they are) and the
 *   counters; set_state with w refreshes the fp32 copy.  ti_adw_train_set_lr: the learning rate of the following steps (> 0).
 * Checks of ti_adw_train_grad / ti_adw_train_steps, before any device work, in this order: every descriptor check of ti_adw_vloss in
 *   its order (through the given t); B > TI_ADW_TRAIN_MAX_B (TI_E_UNSUPPORTED); steps: n_steps < 1, one of idx0 / idx1 NULL, no
 *   indices with n_steps != 1, a given t or z with n_steps != 1, n0 or n1 < 1 (without indices: < B); a NULL x0, x1, beta0 or beta1;
 *   TI_CENTER_BATCH / TI_CENTER_MOLECULE (TI_E_UNSUPPORTED); steps: a host index outside its set (TI_E_ARG; device indices are read
 *   back and checked before anything is enqueued); a NULL or non-trainer handle.
 * TI_ADW_TRAIN_MAX_B bounds the activation workspace: 2 * (2B L + 2B) * H fp32 values (y and silu' of net's L hidden layers on 2B
 *   rows and of beta_embed's two on B) are 1.5 GiB at B = 2^16, H = 256, L = 5, and the weight-gradient slices 2B / 512 * n_weights *
 *   4 bytes = 340 MB. */
#define TI_ADW_TRAIN_MAX_B 65536
typedef struct ti_adw_train_desc {
    double  lr, beta1, beta2, eps, weight_decay;   /* torch.optim.Adam: lr, betas = (0.9, 0.999), eps = 1e-8, weight_decay = 0 */
    double  max_grad_norm;                         /* clip_grad_norm_; <= 0 or inf: no clipping */
} ti_adw_train_desc;
ti_handle* ti_adw_trainer_create(const ti_adw_desc* desc, int32_t dim, const double* weights, size_t n_weights,
                                 const ti_adw_train_desc* train, int device);
int ti_adw_train_grad(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* beta0, const float* beta1,
                      const float* t, const float* z, int64_t B, double* out_loss, double* out_mean, double* out_grad, double* out_gnorm,
                      int mem);
int ti_adw_train_apply(ti_handle* h, const double* grad, int32_t* out_skipped);
int ti_adw_train_steps(ti_handle* h, const ti_vloss_desc* desc, const float* x0, int64_t n0, const float* x1, int64_t n1,
                       const float* beta0, const float* beta1, const int64_t* idx0, const int64_t* idx1, const float* t, const float* z,
                       int64_t B, int64_t n_steps, double* out_loss, int64_t* out_skipped, int mem);
int ti_adw_train_get_state(ti_handle* h, double* w, double* m, double* v, int64_t* n_applied, int64_t* n_skipped);
int ti_adw_train_set_state(ti_handle* h, const double* w, const double* m, const double* v, int64_t n_applied);
int ti_adw_train_set_lr(ti_handle* h, double lr);

/* ---- molecule trainer: cPaiNN trained on the velocity loss, on the device ----------------------------------------------------------
 * The optimiser step of the molecule workflow (mdqm9/train_ambient.py:124-149 and its latent twin): StandardVelocityLoss with
 * LinearInterpolant or OneSidedVelocityLoss with OneSidedLinearInterpolant on cPaiNN, its gradient with respect to every parameter,
 * clip_grad_norm_, torch.optim.Adam with L2 weight decay, the NaN skip.  All three variants, F in {32, 64, 128, 256}, L >= 1, any
 * edge template with E >= 1; uniform batches (one species, no edge mask) -- or per-molecule graphs over the template through
 * ti_painn_train_set_graphs, at the end of this header --, f32, one GPU.  A trainer is a handle of its own kind (3),
 * freed by ti_destroy; every painn / adw / adw-trainer entry point refuses it by its kind check, and the calls below refuse every
 * other handle with TI_E_ARG ("not a painn trainer handle").  It owns the fp64 master weights and both Adam moments, and an fp32
 * working copy in the canonical layout of ti_painn_create (weights.painn_param_spec), refreshed by the optimiser kernel.
 * ti_painn_trainer_create: the checks of ti_painn_create in its order (weights are fp64 here; atom_ids may repeat), the weight count,
 *   then: a precision other than TI_PREC_F32 is TI_E_UNSUPPORTED; n_edges == 0 is TI_E_UNSUPPORTED; the train descriptor's checks
 *   (those of ti_adw_train_desc) are TI_E_ARG.  All before any device call.
 *
 * Rows.  A call evaluates R = 2B molecules [xt+; xt-] (ONE_SIDED: B); the halves share t, cond and the embeddings' inputs.  Node row
 *   n = r A + a, edge row r E + k with k the template edge.
 * Forward.  The states, the drawn t and z, the three centrings, the loss rows l_b and *out_mean = sum_b l_b / (B A) are the
 *   velocity-loss block's above, by the same kernels, on the drift the trainer's own forward pass gives.  That pass keeps every
 *   intermediate in device memory and is made of other kernels than the fused drift: every Linear is one fmaf chain per output over
 *   its inputs in order from +0.0 on v_mfma_f32_16x16x4_f32, the bias added afterwards; LayerNorm (eps 1e-5, biased variance) + SiLU,
 *   the message combine, the per-node sums, the update and the readout are elementwise fp32 kernels.  Its relation to ti_painn_vloss
 *   on an f32 drift handle of the same weights is therefore closeness (fp32 round-off), not identity.
 * Backward.  The gradient is of the MEAN loss: d / d b+- = (b+- - target+-) / (B A), target+- = (x1 - x0) +- gamma'(t) z, in fp64 and
 *   rounded to fp32 once.  The reverse pass runs the forward graph backwards in fp32.  No gradient flows into x, edge_dir, d or the
 *   centring; d||vv|| / dvv is 0 where vv = 0; the last message layer's de chunk and the readout's first output get zero gradient;
 *   silu'(u) = s + silu(u) (1 - s).  A per-node sum (the message sums of the forward pass; s[src] and gates v[src] over a node's
 *   outgoing edges, cross (g x dir) over its incoming ones in the reverse pass) walks the template's edges in order, the identity
 *   term first.  Every reduction over rows -- a bias, a LayerNorm weight or bias, a row of the atom or edge-type table -- is taken in
 *   fp64 from the fp32 terms: 16 accumulators, accumulator p adding rows (tables: molecules) p, p + 16, .. in order from +0.0, then
 *   the accumulators in order; a column sum over rows does so per tile of 2048 rows and adds the tiles in order.  A weight gradient contracts over the rows in slices of 2048 rows (TI_PAINN_TRAIN_SLICE; fixed by the
 *   shapes alone), each slice one fp32 fmaf chain per entry in row order, the slices added in fp64 in slice order from +0.0.  No
 *   atomics: a gradient is a function of the weights and the batch -- including the ORDER of its rows -- and not of the launch, the
 *   memory space of the inputs, or what ran before.
 * Clipping, Adam, NaN skip: as for the adw trainer above, by the same kernels, with the mean's divisor B A.
 * ti_painn_train_grad: loss rows, their mean, the gradient of the mean loss at the current weights and its norm; nothing is updated.
 *   out_loss [B] fp64 [host|device] by mem; out_mean, out_grad [n_weights] (canonical layout), out_gnorm fp64 host; any may be NULL.
 *   cond [B][A][ncond] as ti_painn_vloss takes it (NULL for the single-T variant).  Non-finite values are returned as they are.
 * ti_painn_train_apply: clip + Adam with a GIVEN gradient (host, fp64, canonical layout); *out_skipped = 1 where a non-finite entry
 *   made the step a skipped one.
 * ti_painn_train_step: one optimiser step enqueued on the handle's stream, the gradient staying on the device; it is
 *   ti_painn_train_grad followed by ti_painn_train_apply of its out_grad, bit for bit.  *out_mean: the step's mean loss, NaN where
 *   the step was skipped; *out_skipped 0 / 1.
 * ti_painn_train_get_state / set_state / set_lr: as ti_adw_train_get_state / set_state / set_lr.
 * Checks of ti_painn_train_grad / ti_painn_train_step, before any device work, in this order: every descriptor check of
 *   ti_painn_vloss in its order (through the given t); the workspace of the call above the trainer's max_workspace_bytes
 *   (TI_E_UNSUPPORTED; the text names both numbers); a NULL x0, x1 or (where the variant has temperatures) cond; a NULL or other
 *   handle.
 * ti_painn_train_workspace_bytes: what a call over B molecules of loss kind `kind` (TI_VLOSS_*) needs beside the trainer's state, in
 *   bytes (< 0: an error code).  Everything is stored, nothing recomputed.  With halves = 2 (STANDARD) or 1, Rn = halves B A,
 *   Re = halves B E, Rm = max(Rn, Re):
 *     4 [ Re (4 + F (21 L + 15)) + Rn (F (nE + 23 L + 38) + 19) + 4 F Rm + 3 B A ]        activations and gradient buffers, fp32
 *   + 4 ceil(max(Re, 3 Rn) / 2048) (8 F^2 + 11 F)                                          weight-gradient slices of one block
 *   + 8 (5 F ceil(Rm / 2048) + 6 B A + B + max(3 ceil(B A / 1024), ceil(B / 1024), ceil(n_weights / 1024)))      column-sum tiles,
 *                                                                                          centring, loss rows, tile partials, fp64
 *   with nE = 4, 3, 2 for the ambient, multi-T and single-T variant.  max_workspace_bytes == 0 means
 *   TI_PAINN_TRAIN_DEFAULT_WORKSPACE (32 GiB). */
#define TI_PAINN_TRAIN_SLICE 2048
#define TI_PAINN_TRAIN_DEFAULT_WORKSPACE (32ull << 30)
typedef struct ti_painn_train_desc {
    double   lr, beta1, beta2, eps, weight_decay;  /* torch.optim.Adam: lr, betas = (0.9, 0.999), eps = 1e-8, weight_decay = 0 */
    double   max_grad_norm;                        /* clip_grad_norm_; <= 0 or inf: no clipping */
    uint64_t max_workspace_bytes;                  /* the largest workspace a call may take; 0: TI_PAINN_TRAIN_DEFAULT_WORKSPACE */
} ti_painn_train_desc;
ti_handle* ti_painn_trainer_create(const ti_painn_desc* desc, const double* weights, size_t n_weights, const int32_t* edge_src,
                                   const int32_t* edge_dst, const int32_t* edge_type, const int32_t* atom_ids,
                                   const ti_painn_train_desc* train, int device);
int ti_painn_train_grad(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* cond, const float* t,
                        const float* z, int64_t B, double* out_loss, double* out_mean, double* out_grad, double* out_gnorm, int mem);
int ti_painn_train_apply(ti_handle* h, const double* grad, int32_t* out_skipped);
int ti_painn_train_step(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* cond, const float* t,
                        const float* z, int64_t B, double* out_mean, int32_t* out_skipped, int mem);
int ti_painn_train_get_state(ti_handle* h, double* w, double* m, double* v, int64_t* n_applied, int64_t* n_skipped);
int ti_painn_train_set_state(ti_handle* h, const double* w, const double* m, const double* v, int64_t n_applied);
int ti_painn_train_set_lr(ti_handle* h, double lr);
int64_t ti_painn_train_workspace_bytes(ti_handle* h, int64_t B, int32_t kind);

/* ---- molecule trainer, whole epochs: resident sets, many steps a call, base samples drawn on the device -----------------------------
 * ti_painn_train_steps: n_steps steps of a painn trainer handle enqueued on its stream with ONE host synchronisation, at the end.
 *   x0 [n0,A,3] and x1 [n1,A,3] are the resident sets, temp0 [n0] and temp1 [n1] one temperature per molecule (the reference repeats
 *   it over the atoms); all four, and the indices, live in host or device memory by mem.  Step k takes rows idx0[kB .. kB+B-1] of set 0
 *   and idx1[..] of set 1 (int64), gathered on the device into the buffers the passes of ti_painn_train_step read; the same kernel
 *   writes the conditioning: ambient cond[b][a] = (temp0[idx0], temp1[idx1]), multi-T latent cond[b][a] = temp1[idx1] (temp0 is not
 *   read), single-T none (both temperature pointers must be NULL).  idx0 == idx1 == NULL: n_steps must be 1 and the step uses rows
 *   0..B-1.  The call takes no t and no z: both are drawn as ti_painn_vloss draws them, with draw = desc->draw + k and id =
 *   desc->traj_offset + row in the minibatch (TI_TDIST_GIVEN is therefore refused by the descriptor check).  A skipped step consumes
 *   its draw index.
 *   Nothing waits inside the call.  The host keeps a mirror of (n_applied, n_skipped), brought up to date at the end of every call that
 *   steps; from it the Adam bias terms of every count that can occur (n_applied + 1 .. n_applied + n_steps) are uploaded once as a
 *   table, which the optimiser kernel indexes by the DEVICE counter (after a skip the next step reads the entry the skipped one did not
 *   use).  The mean loss of step k goes to entry k of a device log; the NaN skip is decided on the device as in ti_painn_train_step.
 *   After the one synchronisation out_loss [n_steps] (fp64 host; NaN where skipped) and *out_skipped (the steps of this call that were
 *   skipped) are copied; either may be NULL.
 *   update == 1, noise == TI_NOISE_GIVEN: the call is, bit for bit, the sequence of ti_painn_train_step calls on the gathered rows
 *   with draw = desc->draw + k -- master weights, both moments, both counters and every loss.
 *   update == 0: forward only.  Only the forward pass and the loss reduction run; weights, moments and counters are untouched, and
 *   out_loss[k] is, bit for bit, the out_mean ti_painn_train_grad returns for that minibatch (non-finite values as they are;
 *   *out_skipped = 0).
 *   track_best == 1: after the loss of step k is known and BEFORE its update, a kernel compares it with the best loss held in device
 *   memory and, where it is strictly smaller, copies the fp64 master weights into the trainer's best_w buffer -- the weights that
 *   produced that loss, as `copy.deepcopy(model) if loss < epoch_best_loss` keeps them, not the updated ones.  A step that is skipped
 *   (its out_loss entry is NaN) never wins.
 *   noise: TI_NOISE_GIVEN takes x0 from set 0.  TI_NOISE_DRAWN / TI_NOISE_ALIGNED (TI_VLOSS_ONE_SIDED only, x0 == NULL; n0, temp0 and
 *   idx0's VALUES are not used, idx0 must still accompany idx1) produce the minibatch's x0 by the kernels of ti_painn_train_noise from
 *   the gathered x1 with draw = desc->draw + k: a call is then, bit for bit, the loop of ti_painn_train_noise and ti_painn_train_step.
 * ti_painn_train_best: the best weights tracked since the last reset: w [n_weights] fp64 host, *loss, *step (the 0-based count of the
 *   winning step among the steps tracked since the last reset, over all calls); any may be NULL.  reset != 0 then forgets them.
 *   TI_E_ARG where no call has tracked since the last reset (or the creation).  Where every tracked step was skipped: *step = -1, *loss
 *   = +inf and w is not written.
 * ti_painn_train_noise: the latent data set's base samples (mdqm9_latent.py:84-105) for B molecules.
 *   Draw:    x0[b,a,c] = N(seed, traj_offset + b, draw, 3a + c), the Philox normal the STANDARD loss uses for z (one-sided losses have
 *            no z, so the slot is free), bit for bit what oracle.normal returns.
 *   Centre:  each molecule minus its mean over the atoms: the sum in fp64 in atom order from +0.0, divided by A, subtracted in fp64.
 *            x1 is never modified (the data sets are centred already).
 *   TI_NOISE_DRAWN:   out_x0 = that fp64 value rounded to fp32 once; x1 is not read and may be NULL.
 *   TI_NOISE_ALIGNED: the proper rotation R (det +1) that minimises sum_a |x1_a - R x0_a|^2 is applied to the centred fp64 x0 in fp64
 *            and the result rounded to fp32 once (scipy's Rotation.align_vectors(x1, x0)).  One thread per molecule, fp64 throughout:
 *            K = sum_a x1_a x0_a^T over the atoms in order; the eigenvectors v_i of K^T K by 12 cyclic Jacobi sweeps over (0,1), (0,2),
 *            (1,2), sorted by eigenvalue; u_1 = K v_1 / |K v_1|, u_2 = K v_2 made orthogonal to u_1 and normalised, u_3 = +-(u_1 x u_2)
 *            with the sign of (K v_3) . (u_1 x u_2); R = u_1 v_1^T + u_2 v_2^T + d u_3 v_3^T with the determinant correction d =
 *            det[u_1 u_2 u_3] det[v_1 v_2 v_3].  out_rot [B,3,3] fp64 (row-major, optional) is R.  Where the two largest eigenvalues of
 *            Horn's matrix coincide (x1 a mirror image with equal small singular values, collinear atoms) the rotation is not unique and
 *            one of the minimisers is returned.
 *   No atomics, a fixed iteration count and order: a molecule's result repeats bit for bit and depends on (seed, traj_offset + b, draw,
 *   its x1) alone -- not on B, its position, or its neighbours in the batch.  x1, out_x0 [B,A,3] fp32 and out_rot by mem.
 * Checks of ti_painn_train_steps, before any device work, in this order: every descriptor check of ti_painn_vloss in its order (with
 *   t == z == NULL); a NULL steps descriptor; n_steps < 1 (or above 2^31 - 1); an unknown update; an unknown noise; an unknown
 *   track_best; noise != GIVEN with a loss kind other than ONE_SIDED; noise != GIVEN with a non-NULL x0; track_best with update == 0;
 *   the workspace of the call above max_workspace_bytes (TI_E_UNSUPPORTED); one of idx0 / idx1 NULL; no indices with n_steps != 1;
 *   n1 < 1 or (noise GIVEN) n0 < 1 (without indices: < B); desc->draw + n_steps - 1 above 2^31 - 1; a NULL x1 or (noise GIVEN) x0; a
 *   missing temp1 (ambient, multi-T) or temp0 (ambient), or a given one on the single-T variant; a host index outside its set (device
 *   indices are read back and checked before anything is enqueued); a NULL or other handle; noise != GIVEN on the ambient variant
 *   (TI_E_UNSUPPORTED: its set 0 is data); TI_NOISE_ALIGNED with A < 3 (TI_E_UNSUPPORTED: the rotation is not unique).  All TI_E_ARG
 *   unless stated.
 * Checks of ti_painn_train_noise, in this order: noise neither DRAWN nor ALIGNED; B < 1; draw < 0; an unknown mem; a NULL out_x0;
 *   ALIGNED with a NULL x1; a NULL or other handle; ALIGNED with A < 3 (TI_E_UNSUPPORTED).
 * State.  ti_painn_train_workspace_bytes is unchanged.  Beside it a trainer that has served these calls holds, until it is destroyed:
 *   the staged sets of a host call 4 (3 A (n0 + n1) + n0 + n1) bytes, the staged indices 16 n_steps B, the gathered minibatch
 *   4 B A (6 + ncond), the loss log 8 n_steps, the bias table 16 n_steps, best_w 8 n_weights + 16, and the noise kernel's centred
 *   fp64 samples 24 B A. */
enum { TI_NOISE_GIVEN = 0, TI_NOISE_DRAWN = 1, TI_NOISE_ALIGNED = 2 };
typedef struct ti_painn_steps_desc {
    int64_t n_steps;
    int32_t update;      /* 1: optimiser steps; 0: forward only, the loss of every minibatch at the current weights */
    int32_t noise;       /* TI_NOISE_*; DRAWN / ALIGNED only with TI_VLOSS_ONE_SIDED, x0 must then be NULL */
    int32_t track_best;  /* 1: keep the master weights of the step with the smallest loss seen since the last reset */
} ti_painn_steps_desc;
int ti_painn_train_steps(ti_handle* h, const ti_vloss_desc* desc, const ti_painn_steps_desc* steps, const float* x0, int64_t n0,
                         const float* temp0, const float* x1, int64_t n1, const float* temp1, const int64_t* idx0, const int64_t* idx1,
                         int64_t B, double* out_loss, int64_t* out_skipped, int mem);
int ti_painn_train_best(ti_handle* h, double* w, double* loss, int64_t* step, int reset);
int ti_painn_train_noise(ti_handle* h, uint64_t seed, int64_t traj_offset, int32_t draw, const float* x1, int64_t B, int32_t noise,
                         float* out_x0, double* out_rot, int mem);

/* ---- molecule trainer on per-molecule graphs: edge masks and mixed species ----------------------------------------------------------
 * ti_painn_train_set_graphs: a table of n per-molecule graphs over the TRAINER's template (handle kind 3; ti_painn_set_edge_mask and
 *   ti_painn_set_molecules keep refusing a trainer), in the conventions of ti_painn_set_molecules: n_atoms [n] each in 1..A (NULL:
 *   every molecule has A atoms), atoms a >= n_atoms[b] are PAD atoms; mask [n][A], bit s of mask[b*A + d] = the edge s -> d exists
 *   (NULL: every template edge between real atoms; s up to 31); pair_type [n][A][A] bytes 0..3, pair_type[(b*A + s)*A + d] the type of
 *   s -> d (NULL: the template's types).  The library clears every bit that touches a pad atom; bits of pairs outside the template
 *   are ignored.  All three NULL clears the table.  The arrays are copied into the handle; `mem` says where all three live.
 *   Checks, before any device work, in this order: a NULL or other handle; n < 1 with a non-NULL array; a count outside 1..A; a type
 *   above 3 (host arrays; device arrays are checked after their copy, before the table changes); an unknown mem.  All TI_E_ARG.
 *   Which row a molecule reads.  ti_painn_train_grad / _step: molecule b uses row b, both halves [xt+; xt-] the row of b = r % B; a
 *   table with n != B is TI_E_ARG.  ti_painn_train_steps with TI_NOISE_GIVEN: minibatch molecule j of step k uses row idx0[kB + j]
 *   (without indices rows 0..B-1) -- the graph is batch0's, as in the reference's loss -- gathered on the device by the kernel that
 *   expands the rows; n != n0 is TI_E_ARG.  Pairing an x1 row of the same species is the caller's business.  A table in force with
 *   TI_NOISE_DRAWN / _ALIGNED is TI_E_UNSUPPORTED.  ti_painn_train_noise is unchanged.
 * Semantics with a table in force (N = sum_b n_atoms[row of b], the real node rows of the call):
 *   Pad atoms.  The passes run on a copy in which pad atom a of molecule b sits at xt[b][0] + (100 (a - n_b + 1), 0, 0) with cond 0 (the
 *     drift's rule above), so every row of the dense layout is finite.  The library never reads a pad entry of x0, x1, cond or z: every
 *     result is bit-identical whatever finite values they hold.
 *   Interpolation and draws run over real entries only; a real component keeps its Philox key (seed, id, draw, 3a + c); pads draw
 *     nothing.  TI_CENTER_BATCH takes the column means over the N real node rows (the reference's mean(dim=0) over its flat [N,3]):
 *     the fp64 scheme above with pad rows entering as +0.0, divided by N.  TI_CENTER_MOLECULE runs over the n_b real atoms.
 *   Loss.  l_b runs over the real entries; *out_mean = sum_b l_b / N; the output gradient is (b - target) / N on real rows and +0 on
 *     pads; clip, Adam and the NaN skip use the divisor N.
 *   Forward.  The edge-embedding row is pair_type[b][s][d]'s where given.  Per-node sums skip DEAD edges: those whose bit is clear or
 *     that touch a pad.  Dead edge rows and pad node rows are computed like any other (finite), nothing reads them into a real row.
 *   Reverse.  The per-node sums skip dead edges; the gP and gWd rows of dead edges are written as +0, so every weight-gradient
 *     product, column sum and LayerNorm reverse receives exact zeros from dead rows and from pad node rows.  The dense products are
 *     not compacted.  The edge-type table gradient is indexed by each molecule's own type per edge.
 *   No atomics: the determinism paragraph above holds as it stands.
 *   Identities, bit for bit: (a) a full table (n_atoms = A or NULL, every template bit set, pair_type NULL) gives the outputs of the
 *     call without a table; (b) with update == 1 and TI_NOISE_GIVEN ti_painn_train_steps is the loop of ti_painn_train_set_graphs on
 *     the gathered rows and ti_painn_train_step.  Without a table every call runs the kernels it ran before.
 * State.  ti_painn_train_workspace_bytes and its formula are unchanged.  Beside the workspace the table takes n (4 + 4 A + A^2) bytes
 *   (n (4 + 4 A) where pair_type is NULL: the types are then not stored) and a call with a table B (E + 4) bytes of per-call flags:
 *   one byte per (molecule, template edge) -- bit 7 dead, bits 0..1 the type -- and the atom count. */
int ti_painn_train_set_graphs(ti_handle* h, const int32_t* n_atoms, const uint32_t* mask, const uint8_t* pair_type, int64_t n, int mem);

#ifdef __cplusplus
}
#endif
#endif /* TI_HIP_H */
