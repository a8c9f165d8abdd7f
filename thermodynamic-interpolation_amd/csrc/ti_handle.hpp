// ti_handle.hpp -- private header of the host side of libti_hip.so: error plumbing, device buffers, the handle behind the C ABI
// (include/ti_hip.h), the staging of host-resident arguments, and the host functions the units call across each other:
//   painn_pack.hip   weight packing, edge templates          painn_host.hip   PaiNN workspace, drift / divergence drivers, graph state
//   rollout.hpp      the integrator drivers (templates)      api_*.hip        the extern "C" entry points
// The observables' entry points by unit:
//   api_obs.hip           states or log-weights into per-sample numbers and histograms (CVs and the observer, weights, histograms,
//                         TI and Boltzmann-generator log-weights); the reductions the other units share (obs_scratch, logw_shift_dev)
//   api_obs_resample.hip  bootstrap intervals, RFF Gram matrices of resamples
//   api_obs_eig.hip       both eigensolvers, both gEDMD spectra
//   api_obs_zmat.hip      Z-matrix coordinates both ways
//   api_obs_tica.hip      TICA: lagged moments, the model, the projection
//   api_ff.hip            the force field: tables, energies, forces, Langevin dynamics, replica exchange
//
// There is deliberately no CPU fallback in the host code: every entry point either runs the HIP kernels or fails.
#pragma once
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ti_internal.hpp"

namespace ti {

int fail(int code, const std::string& msg);      // sets the calling thread's ti_last_error() text (api_common.hip), returns code

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };      // -> TI_E_UNSUPPORTED (guarded)
#define HIP_CHECK(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) \
    throw HipError(std::string(#expr) + ": " + hipGetErrorString(e__)); } while (0)

// refusals more than one entry point gives
constexpr const char* MSG_NO_FP16_TANGENT = "the fp16 storage mode has no divergence / tangent path (use f32 or f16x2)";
constexpr const char* MSG_TRAJ_OBSERVER = "TI_SCHEME_DOPRI5_TRAJ writes its rows per trajectory inside a kernel: detach the observer (ti_obs_set_observer)";
constexpr const char* MSG_TAP_ENTRIES = "debug taps apply to ti_painn_drift / ti_painn_drift_jvp only";
constexpr const char* MSG_EM_DLOGP = "dlogp is defined for a deterministic flow: EM needs eps = 0";

struct MlpOff { size_t W0, b0, g0, be0, W1, b1, g1, be1, W2, b2; int f_in, f_h, f_out; };

template <typename T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;
    void alloc(size_t count) { release(); if (count) { HIP_CHECK(hipMalloc((void**)&p, count * sizeof(T))); n = count; } }
    void upload(const std::vector<T>& h) { alloc(h.size()); if (n) HIP_CHECK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice)); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
    ~DevBuf() { release(); }
};

template <typename T>
void grow(DevBuf<T>& b, size_t n) { if (b.n < n) b.alloc(n); }      // grow-on-demand scratch: never shrinks, contents are not kept

struct Stream { size_t off4; int nch; };      // offset into the packed buffer in float4 units

}  // namespace ti

using namespace ti;

// ====================================================================================================== handle
struct ti_handle {
    int kind = 0;                 // 0 painn, 1 adw, 2 adw trainer (api_adw_train.hip), 3 painn trainer (api_painn_train.hip), both on train_optim.hpp; every painn / adw entry point refuses a trainer by kind
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t wait_ev = nullptr;          // ti_wait_stream
    // profiling
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[TI_KERNEL_COUNT];
    // common device buffers
    DevBuf<float> flat, packed;
    DevBuf<int> nanflag;
    long long cap = 0;            // trajectories the workspace is sized for

    // ---- painn
    ti_painn_desc d{};
    int NB = 0, nE = 0, ncond = 0, G = 1, nblk = 0, n_tile = 0;
    MlpOff embed{}, readout{}; std::vector<MlpOff> phi, w, upd; std::vector<size_t> U, V;
    size_t edge_emb = 0, atom_emb = 0, Vr = 0; float b2_gate = 0.f;
    Stream st_embed16{}; std::vector<Stream> st_edge, st_edge1, st_update;      // st_edge1: the message kernel's one-accumulator format (TI_PREC_F16X2)
    // edge templates (ti_internal.hpp): [0] throughput (G molecules per group), [1] latency (G = 1, P parts per molecule);
    // G / P / nblk / rows / slotnode below are those of the ACTIVE one (select_template, once per API call)
    struct Tpl {
        int G = 1, P = 1, nblk = 0;
        int n_tile = 0;                           // pair template: its leading tile blocks, the rest are general (pair_template.hpp)
        DevBuf<uint32_t> rows; DevBuf<int32_t> slotnode;
        std::vector<uint32_t> rows_h;             // host copy of `rows` (masked_rows)
        std::vector<int> part_of, part_start, part_len;     // per sorted edge: its part; per part: first sorted edge, edges
        std::vector<int> pos;                     // row of (molecule-in-group m, sorted edge k) inside its part: pos[m * part_len + (k - part_start)]
        int max_slots = 0;                        // most destination atoms in any row block (<= EDGE_MAX_SLOTS)
    } tpl[3];
    // tpl[2]: the pair-major template (ti_internal.hpp; painn_pair_kernel.hpp), built when the graph is symmetric and the pair kernel
    // exists for this width / precision: the packed one (tile blocks, then general blocks), or with TI_PAIR_PACKED=0 in the environment
    // at creation the tile-only one of before (same-binary A/B runs, triage).  pair_pos[(m * A + src) * A + dst] = e row of that directed edge of molecule-in-group m inside
    // its group: (block * 2 + direction) * 16 + pair row
    bool has_pair = false; std::vector<int> pair_pos; double pair_fill = 0.0;
    // seeded accumulators.  pair_seeded: the pair template's general rows name every atom of a group exactly once
    // (pair_template.hpp: pair_template_seeded).  pair_seeded_on: the handle may then run the general launch of a layer first, with
    // plain stores, and tile launches that only add -- unless TI_PAIR_SEEDED=0 was in the environment at creation (same-binary A/B
    // runs, triage).  Plain split-path evaluations only (painn_host.hip).  seeded_last: what ti_painn_debug_pair_seeded reports.
    bool pair_seeded = false, pair_seeded_on = false; int seeded_last = -1;
    // merged tails (pair_template.hpp: pair_template_tails).  pair_tail_S / pair_tail_r: groups per super-group and valid rows of the
    // last general block, 0 when the template has none the kernel takes.  pair_tails_on: the seeded general launch then walks super-
    // groups, the S last blocks as one -- unless TI_PAIR_TAILS=0 was in the environment at creation.  tails_last: what
    // ti_painn_debug_pair_tails reports.
    int pair_tail_S = 0, pair_tail_r = 0; bool pair_tails_on = false; int tails_last = -1;
    int n_tpl = 1, active = 0, parts = 1, max_slots = 0, pinned_tpl = TI_TEMPLATE_AUTO;
    // every atom has incoming edges: the edge kernels' first touch of an accumulator replaces its contents (ti_internal.hpp
    // SLOT_FIRST_TOUCH) and nothing zeroes the accumulators between layers or calls; otherwise the update kernel zeroes them as before
    bool first_touch = false;
    // per-molecule edge sets (ti_painn_set_edge_mask): [emask_B][A] words, in force for calls over emask_B molecules (0: no mask);
    // emask_sym: every molecule's set is symmetric over the template (the pair layout is eligible).  mrows[t]: the row words of
    // template t per (group, part) of those molecules with the absent edges switched off (masked_rows), built on first use.
    std::vector<uint32_t> emask; long long emask_B = 0; bool emask_sym = true;
    // emask_full: the state in force removes nothing -- every template edge of every molecule is present, no per-molecule edge types, no
    // pad atoms -- so its row words are the template's (painn_host.hip: a seeded pair layout then keeps the launches of an unmasked batch)
    bool emask_full = false;
    DevBuf<uint32_t> mrows[3]; bool mrows_ok[3] = {false, false, false};
    // mixed species (ti_painn_set_molecules), part of the same per-molecule graph state: natoms [emask_B] atom counts (empty: all A),
    // ptype [emask_B][A][A] edge types (empty: the template's).  ragged: some molecule has pad atoms -- only then the drift runs on
    // parked copies of x / cond / xdot (xpark, cpark, dpark), zeroes the pad rows of its outputs, and the integrators take their
    // ragged twins; natoms_dev is the device copy of natoms the kernels read.
    std::vector<int32_t> natoms; std::vector<uint8_t> ptype; bool ragged = false; long long n_real = 0;
    DevBuf<int32_t> natoms_dev; DevBuf<float> xpark, cpark, dpark;
    struct { const uint32_t* p = nullptr; } rows; struct { const int32_t* p = nullptr; } slotnode;
    DevBuf<int32_t> atom_ids;
    std::vector<int> perm;        // sorted row -> original edge index
    std::vector<int32_t> esrc, edst;       // the molecule's directed edges as passed to create
    DevBuf<float> x, cond, s, P, v, dsacc, dvacc, cacc, e, enc, geo, b1, b2, xt, edge_vecs, edge_vecs1, upd_vecs;
    std::vector<float> edge_scale;               // [L][6] per-matrix powers of two of the one-accumulator message streams (TI_PREC_F16X2)
    int tap = -1; long long last_B = 0;
    // layer-0 phi table (painn_phi0_kernels.hip).  phi0_ok: the handle can take the table path at all (pair layout, a
    // table build of the pair kernel, TI_PHI0_TABLE != 0 at creation); st_phi0_w / st_phi0_tab: layer 0's message stream cut in two,
    // the w chunks in the table build's walk order (phi0_wpad: it ends with a pad chunk) and the phi chunks in the table kernel's.
    // Per API call (phi0_begin_call ... phi0_end_call): phi0_cls [B] class ids and phi0_state (representatives, overflow flag) from
    // the class pass, phi0_ncls the class count read back from it (0: no class pass, or more classes than the cap), for phi0_B
    // molecules whose cond rows start at phi0_cond.  phi0_last: what ti_painn_debug_phi0_path reports.
    bool phi0_ok = false; Stream st_phi0_w{}, st_phi0_tab{}; int phi0_wpad = 0;
    DevBuf<uint8_t> phi0_cls; DevBuf<int32_t> phi0_state; DevBuf<float> phi0_tab;
    int phi0_ncls = 0, phi0_found = 0, phi0_last = -1; long long phi0_B = 0; const float* phi0_cond = nullptr;
    // embed per class: on the table path only the table kernel (P of the representatives) and layer 0's update (s, once)
    // read the embedding, and the rows of a class agree bit for bit.  embed_cls_on: the embed launch of such an evaluation then covers
    // the classes alone -- s_cls / P_cls [class][atom][F] -- and layer 0's update reads s through phi0_cls; the full s / P are first
    // written by that update.  Off with TI_EMBED_CLASSES=0 in the environment at creation (same-binary A/B runs, triage).
    // embed_cls_last: what ti_painn_debug_embed_path reports.
    bool embed_cls_on = false; int embed_cls_last = -1; DevBuf<float> s_cls, P_cls;
    // update launches on the builds that keep v_eff in registers (painn_update_keep.hip): the split
    // path up to F = 128.  Off with TI_UPDATE_KEEP=0 in the environment at creation (same-binary A/B runs, triage).
    // update_keep_last: what ti_painn_debug_update_keep reports.
    bool update_keep_on = false; int update_keep_last = -1;
    // forward-mode derivative (painn_jvp_kernels.hip): tangent twins over virtual molecules, sized on first use
    std::vector<Stream> st_jvp_update, st_jvp_phi; Stream st_jvp_readout{}; std::vector<int> jvp_phi_pad;
    DevBuf<float> jvp_ro_vecs, ts, tP, tv, tdsacc, tdvacc, tcacc, te, tout, wq, phist, nodest, divb, dl, dlscaled, div2;
    long long jvp_cap = 0, last_VB = 0; int last_D = 1;
    DevBuf<float> probes;                        // Hutchinson probes of the current call [B][k][3A] (painn_make_probes)
    // Runge-Kutta drivers (rollout_rk): stage derivatives, dense-output coefficients, reduction scratch
    DevBuf<float> rk_ws; DevBuf<double> rk_red;
    // per-trajectory dopri5 (rollout_rk_traj): controller state, stage times, status words, grid, host-output staging, and the
    // accepted / rejected counts of the last such rollout (ti_rollout_step_counts)
    DevBuf<TrajCtl> rk_ctl; DevBuf<float> rk_tv, rk_path, rk_dpath; DevBuf<int> rk_status; DevBuf<double> rk_grid;
    std::vector<int64_t> traj_accepted, traj_rejected;

    // ---- adw
    ti_adw_desc ad{};
    size_t a_be_vecs = 0, a_net_vecs = 0;          // offsets of the per-MLP vector blocks in `flat`
    float a_be_b_out = 0.f, a_b_out = 0.f;
    int a_dim = 1;                                 // d of FCNetMultiBeta(d, d, H, L): floats per particle of x / b
    Stream st_be{}, st_net{};
    DevBuf<float> ax, ab1, ab2, axt, aemb_u, abeta0_u, abeta1_u, adl, ad1, ad2; DevBuf<int32_t> aidx;
    DevBuf<float> abeta0_r, abeta1_r, aemb_r, atv;                  // per-row conditioning / beta embedding / times (per-row t)
    // fused rollout (ti_adw_rollout_fused): embedding-table inputs [n_step * U] and the table itself, the per-step scalars, and the
    // saved rows of a TI_MEM_HOST call (path, dlogp) ahead of their one copy
    DevBuf<float> af_b0, af_b1, af_tv, af_emb, af_path, af_dl; DevBuf<AdwFusedStep> af_steps;

    // ---- observables (ti_obs_*): descriptor sets as validated and uploaded by obs_upload -- [0] of the last ti_obs_cv call, [1] the
    // attached observer (K == 0: none) with its row stride `every` and the caller's out_cv; staging for host buffers; fp64 scratch:
    // red = (max, first bad index, sum w, sum w^2, hist [n_bins + 3]), part = per-block partials
    struct ObsSet { int K = 0; bool has_ref = false, has_sel = false; DevBuf<int32_t> desc, sel; DevBuf<float> ref; } obs[2];
    int obs_every = 0, obs_mem = TI_MEM_HOST; float* obs_out = nullptr;
    DevBuf<float> obs_x, obs_cv, obs_val, obs_logw, obs_w; DevBuf<double> obs_red, obs_part;
    // bootstrap (ti_obs_bootstrap): the once-filtered population, staged index rows, the estimates ahead of their validation, the
    // point row's (estimate, kept count, lower and upper filter bound, size of the compacted population), the bad-index flag
    DevBuf<float> boot_pop; DevBuf<int32_t> boot_idx; DevBuf<double> boot_est, boot_pt; DevBuf<int> boot_flag;
    // RFF Gram matrices (ti_obs_rff_gram): the packed values of a host call, Omega, the feature table, the weights, the partial
    // tiles of one launch, the result ahead of its validation
    DevBuf<float> gram_x; DevBuf<double> gram_omega, gram_z, gram_w, gram_part, gram_out;
    // eigensolver and gEDMD algebra (ti_obs_eigh, ti_obs_gedmd_spectrum): the staged input of a host call; eigenvalues, eigenvectors and
    // status words of the first and second solve; K, the reduced matrices of one launch, the ranks; the results ahead of their validation
    DevBuf<double> eig_a, eig_w, eig_v, eig_w2, eig_v2, eig_k, eig_r, eig_ev, eig_vec; DevBuf<int32_t> eig_st, eig_st2, eig_rank;
    // blocked eigensolver and wide gEDMD algebra (ti_obs_eigh_wide, ti_obs_gedmd_spectrum_wide): A, V, the pair rotations and swept
    // blocks, thresholds and flag words of one launch; the singular values, L, T, the per-solver orders and the status words of the
    // second solve by either kernel
    DevBuf<double> eigw_a, eigw_v, eigw_u, eigw_s, eigw_thr, eigw_sv, eigw_l, eigw_t;
    DevBuf<int32_t> eigw_rot, eigw_prot, eigw_st, eigw_nvn, eigw_nvw, eigw_live, eigw_st2n;
    // force field (ti_obs_ff_set; painn handles): the term words and parameters of the four tables as validated and packed by the
    // host (ti_internal.hpp FfParams), their lengths (ff_on: a force field is in force); staging of a host call's temperatures,
    // energies, term sums, reduced energies and log-weights (ti_obs_ff_energy, ti_obs_ti_logw)
    bool ff_on = false; int ff_n[4] = {0, 0, 0, 0}; double ff_coulomb = 0.0;
    DevBuf<int32_t> ff_idx; DevBuf<double> ff_par, ff_e, ff_terms, ff_u0, ff_u1; DevBuf<float> ff_T;
    // Boltzmann-generator log-weights (ti_obs_bg_logw): staging of a host call's second dlogp and of log p(z); the rest of its
    // buffers are those of the calls above (obs_x, ff_u1, obs_val, obs_logw)
    DevBuf<float> bg_nt; DevBuf<double> bg_logpz;
    // forces and Langevin dynamics (ti_obs_ff_forces, ti_obs_ff_set_masses, ti_obs_ff_langevin): the incidence list of the bonded
    // terms, built with the force field (ff_device.hpp); the masses (ff_mass_on: in force; cleared with the force field); staging of a
    // host call's forces; the working copy of the state, the replica ids, frames, frame energies and stop flags of a Langevin call
    DevBuf<int32_t> ff_inc; bool ff_mass_on = false;
    DevBuf<double> ff_mass, ff_f, md_pos, md_vel, md_epot, md_ekin; DevBuf<float> md_frames; DevBuf<int64_t> md_ids; DevBuf<int> md_flag;
    // replica exchange (ti_obs_ff_remd): the ladder ids, the working copy of the walker labels, and staging of a host call's walker
    // history and pair counts
    DevBuf<int64_t> md_ladder_ids, md_counts; DevBuf<int32_t> md_walker, md_walker_in, md_out_walker;
    // Z-matrix coordinates and column histograms (ti_obs_zmat, ti_obs_zmat_xyz, ti_obs_hist_cols): the topology of the call (order,
    // ref), staging of a host call's z, log-determinants, validity and keep masks, the column ranges (lo [K], hi [K])
    DevBuf<int32_t> zm_topo; DevBuf<float> zm_z; DevBuf<double> zm_logdet, hc_range; DevBuf<uint8_t> zm_valid, hc_keep;
    // TICA (ti_obs_tica_moments, ti_obs_tica_fit, ti_obs_tica_transform): the packed values of a host call; the feature table, the
    // partial tiles of one launch, the moments ahead of their validation; traj_off, the cumulative pair counts of one launch, the
    // per-block and the first bad row; the staged moments of a host fit, C0t, L and the model ahead of its validation; the staged
    // model and the output of a host transform.  The solves use the eig_* buffers above.
    DevBuf<float> tica_x, tica_y; DevBuf<double> tica_f, tica_part, tica_sum, tica_cov, tica_c0t, tica_l, tica_mean, tica_ev, tica_comp;
    DevBuf<long long> tica_off, tica_cum, tica_bad, tica_cnt; DevBuf<int32_t> tica_flag;
    // velocity loss (ti_painn_vloss, ti_adw_vloss): every stage computes into these and the outputs are copied from them at the end.
    // Staged inputs of a host call (x0, x1, z, conditioning); the times, the noise, the states [2][B][m] and the drift on them; the
    // times and conditioning of the evaluated batch (both halves, with the pad molecules of a packed layout); the uncentred states, the tile partials, (column sums [32], mean, first
    // bad index, time profile) and the losses
    DevBuf<float> vl_x0, vl_x1, vl_zin, vl_c0, vl_c1, vl_t, vl_z, vl_xt, vl_b, vl_t2, vl_c02, vl_c12;
    DevBuf<double> vl_raw, vl_part, vl_red, vl_loss;

    // ---- trainers (kind 2, 3): the AdwTrainState / PainnTrainState of api_adw_train.hip / api_painn_train.hip (either an Optim of
    // train_optim.hpp with the trainer's own buffers), owned here so that ti_destroy frees it with the handle
    std::shared_ptr<void> train;

    ~ti_handle()
    {
        for (auto& v2 : ev) for (auto& pr : v2) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        if (wait_ev) (void)hipEventDestroy(wait_ev);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
    const float* F(size_t off) const { return flat.p + off; }
    const float4* S(const Stream& s2) const { return reinterpret_cast<const float4*>(packed.p) + s2.off4; }
    MlpVec vec(const MlpOff& m) const { return MlpVec{F(m.b0), F(m.g0), F(m.be0), F(m.b1), F(m.g1), F(m.be1), F(m.b2)}; }
};

namespace ti {

struct Timed {           // RAII: brackets a launch with HIP events when profiling is on
    ti_handle* h; int slot; hipEvent_t a = nullptr, b = nullptr;
    Timed(ti_handle* h_, int slot_) : h(h_), slot(slot_)
    {
        if (!h->prof) return;
        HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b));
        HIP_CHECK(hipEventRecord(a, h->stream));
    }
    ~Timed()
    {
        if (!a) return;
        (void)hipEventRecord(b, h->stream);
        h->ev[slot].emplace_back(a, b);
    }
};

inline void set_device(const ti_handle* h) { HIP_CHECK(hipSetDevice(h->device)); }

template <typename Fn>
int guarded(Fn&& fn)
{
    try { return fn(); }
    catch (const HipError& e) { return fail(TI_E_HIP, e.what()); }
    catch (const Unsupported& e) { return fail(TI_E_UNSUPPORTED, e.what()); }
    catch (const std::bad_alloc&) { return fail(TI_E_ALLOC, "host allocation failed"); }
    catch (const std::exception& e) { return fail(TI_E_ARG, e.what()); }
}

inline ti_handle* new_handle(int kind, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw HipError("no HIP device available (libti_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) throw std::invalid_argument("device index out of range");
    HIP_CHECK(hipSetDevice(device));
    std::unique_ptr<ti_handle> h(new ti_handle());
    h->kind = kind; h->device = device;
    HIP_CHECK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    h->nanflag.alloc(1);
    return h.release();
}

// The arguments of one API call that live where `mem` says.  TI_MEM_DEVICE: every pointer is used as it is.  TI_MEM_HOST: in()
// mirrors an input in a buffer of the handle (the copy is enqueued on the handle's stream at once), out() hands out the buffer to
// compute into, and finish() copies those back in the order they were asked for.  finish() ends the call: it synchronises the stream.
struct Staged {
    ti_handle* h; bool host;
    struct { void* dst; const void* src; size_t bytes; } back[3] = {}; int n_back = 0;
    Staged(ti_handle* h_, int mem) : h(h_), host(mem == TI_MEM_HOST) {}
    template <typename T>
    const T* in(const T* p, DevBuf<T>& b, size_t n)
    {
        if (!host || !p) return p;          // an optional input that is absent stays NULL (the trainers' t, z, sets)
        grow(b, n);
        if (n) HIP_CHECK(hipMemcpyAsync(b.p, p, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
        return b.p;
    }
    template <typename T>
    T* out(T* p, DevBuf<T>& b, size_t n)
    {
        if (!host) return p;
        grow(b, n);
        back[n_back++] = {p, b.p, n * sizeof(T)};
        return b.p;
    }
    // The first d columns of the n rows of p, `stride` floats apart.  TI_MEM_HOST: packed densely into b, so that only they cross the
    // bus (a blocking copy: the packed rows are a pageable temporary), and stride becomes d.
    const float* in_cols(const float* p, long long& stride, long long n, int d, DevBuf<float>& b)
    {
        if (!host) return p;
        std::vector<float> rows((size_t)n * d);
        for (long long i = 0; i < n; ++i) std::copy(p + i * stride, p + i * stride + d, rows.begin() + i * d);
        grow(b, rows.size());
        HIP_CHECK(hipMemcpy(b.p, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
        stride = d;
        return b.p;
    }
    void finish(bool copy_back = true)
    {
        for (int i = 0; copy_back && i < n_back; ++i) HIP_CHECK(hipMemcpyAsync(back[i].dst, back[i].src, back[i].bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }
};

// the direction of a copy between the handle's buffers and a caller's array that lives where `mem` says, for the calls that copy by hand
inline hipMemcpyKind in_kind(int mem) { return mem == TI_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice; }
inline hipMemcpyKind out_kind(int mem) { return mem == TI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice; }

struct JvpRun {            // one tangent pass riding on a drift evaluation
    int D;                 // seed directions per molecule
    const float* xdot;     // D explicit directions [B][D][A][3] (device; D = 1: ti_painn_drift_jvp, D = k: Hutchinson probes); NULL: unit seeds, D = 3A
    float* tout;           // [B*D*A*3] tangent of the drift (device)
};

inline int obs_floats_per_traj(const ti_handle* h) { return h->kind == 0 ? 3 * h->d.n_atoms : h->a_dim; }

// ---- painn_pack.hip
void pack_chunk16(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK);
void pack_chunk16_split(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK);
size_t take_mlp(MlpOff& m, size_t o, int f_in, int f_h, int f_out);
void pack_painn(ti_handle* h, const float* wts);
void build_templates(ti_handle* h, const int32_t* src, const int32_t* dst, const int32_t* etype);
bool build_pair_template(ti_handle* h, const int32_t* src, const int32_t* dst, const int32_t* etype);
int pinned_template(const ti_handle* h);
bool mask_blocks_pair(const ti_handle* h);
int template_for(const ti_handle* h, long long B, bool allow_pair = true);
void select_template(ti_handle* h, long long B, bool allow_pair = true);
const uint32_t* masked_rows(ti_handle* h, int t);
size_t edge_row_of(const ti_handle* h, size_t m, size_t k);
size_t edge_rows_for(const ti_handle* h, long long B, long long copies = 1);

// ---- painn_host.hip
void ensure_painn_ws(ti_handle* h, long long B);
void ensure_jvp_ws(ti_handle* h, long long B, int D);
void painn_drift_dev(ti_handle* h, const float* x_dev, float t, const float* cond_dev, long long B, float* out_dev,
                     const JvpRun* jr = nullptr, const float* tv = nullptr, long long b0 = 0);
void painn_drift_div_dev(ti_handle* h, const float* x_dev, float t, const float* cond_dev, long long B, float* out_dev, float* div_dev,
                         const float* tv = nullptr);
void painn_make_probes(ti_handle* h, long long B, int k, uint64_t seed, long long traj0);
void painn_drift_div_est_dev(ti_handle* h, const float* x_dev, float t, const float* cond_dev, long long B, int k, float* out_dev,
                             float* est_dev, const float* tv = nullptr);
// the class pass of an API call over B molecules with cond rows cond_dev (device), where the call (eligible: one t for all molecules,
// no tangent pass) and the handle's state allow the table path at all; phi0_end_call forgets its result (the next call's cond may differ)
void phi0_begin_call(ti_handle* h, const float* cond_dev, long long B, bool eligible);
void phi0_end_call(ti_handle* h);
int set_graph_state(ti_handle* h, std::vector<uint32_t>& m, std::vector<int32_t>& natoms, std::vector<uint8_t>& ptype, long long B);
void clear_graph_state(ti_handle* h);

// ---- api_adw.hip, api_obs.hip: what ti_reserve, the rollout drivers, the velocity loss and the other observables units need of them
void ensure_adw_ws(ti_handle* h, long long B);
void adw_drift_tv_dev(ti_handle* h, const float* x_dev, const float* tv, const float* beta0, const float* beta1, long long B, float* out_dev,
                      float* out_div);
void obs_cv_dev(ti_handle* h, int which, const float* x_dev, long long B, float* cv_dev);
void obs_scratch(ti_handle* h, size_t words = 259);
int logw_shift_dev(ti_handle* h, const float* logw_dev, long long n, double out[2]);

}  // namespace ti
