// ti_api.hip -- host side of libti_hip.so: C ABI (include/ti_hip.h), weight packing, edge templates, HBM workspace,
// drift / rollout orchestration on one HIP stream, live kernel timing with HIP events.
//
// There is deliberately no CPU fallback in this file: every entry point either runs the HIP kernels or fails.
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
#include <utility>

#include "pair_template.hpp"
#include "ti_internal.hpp"

namespace ti {

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };      // -> TI_E_UNSUPPORTED (guarded)
#define HIP_CHECK(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) \
    throw HipError(std::string(#expr) + ": " + hipGetErrorString(e__)); } while (0)

// ---------------------------------------------------------------------------------------------------- packing
// 16-row kernels (mfma_chain.hpp, namespace r16): chunk[(blk*NBK + nbi)*64 + l][r] = W[row0 + 16*blk + (l&15)][col0 + 16*nbi + 4*(l>>4) + r]
void pack_chunk16(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)2 * NBK * 64 * 4);
    for (int blk = 0; blk < 2; ++blk)
        for (int nbi = 0; nbi < NBK; ++nbi)
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + 16 * blk + (l & 15), col = col0 + 16 * nbi + 4 * (l >> 4) + r;
                    dst[base + ((size_t)(blk * NBK + nbi) * 64 + l) * 4 + r] = row < n_rows ? W[(size_t)row * ld + col] : 0.f;
                }
}

// split-fp16 chunk of the edge kernel (mfma_chain.hpp, r16::Opnd<NBK,true>): 16-byte h8 fragments
//   frag[((blk*(NBK/2) + m)*2 + {0 hi, 1 lo})*64 + l][i] = half of W[row0 + 16*blk + (l&15)][col0 + 16*(2m + (i>>2)) + 4*(l>>4) + (i&3)]
// with hi = fp16(w), lo = fp16((w - hi) * 2^11).  Same byte size as the fp32 chunk.
void pack_chunk16_split(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)2 * NBK * 64 * 4);
    _Float16* out = reinterpret_cast<_Float16*>(dst.data() + base);
    const int KS = NBK / 2;
    for (int blk = 0; blk < 2; ++blk)
        for (int m = 0; m < KS; ++m)
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < 8; ++i) {
                    const int row = row0 + 16 * blk + (l & 15), col = col0 + 16 * (2 * m + (i >> 2)) + 4 * (l >> 4) + (i & 3);
                    const float w = row < n_rows ? W[(size_t)row * ld + col] : 0.f;
                    const _Float16 h = (_Float16)w;
                    const _Float16 lo = (_Float16)((w - (float)h) * 2048.0f);
                    out[((size_t)((blk * KS + m) * 2 + 0) * 64 + l) * 8 + i] = h;
                    out[((size_t)((blk * KS + m) * 2 + 1) * 64 + l) * 8 + i] = lo;
                }
}

// one-accumulator format of the message kernel (mfma_chain.hpp: Opnd1 / gemm_split_chunk1): the matrix is scaled by the power of two S
// first and the residual is NOT scaled:  hi = fp16(S w), lo = fp16(S w - hi).  Same layout and size as pack_chunk16_split.
void pack_chunk16_split1(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK, float S)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)2 * NBK * 64 * 4);
    _Float16* out = reinterpret_cast<_Float16*>(dst.data() + base);
    const int KS = NBK / 2;
    for (int blk = 0; blk < 2; ++blk)
        for (int m = 0; m < KS; ++m)
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < 8; ++i) {
                    const int row = row0 + 16 * blk + (l & 15), col = col0 + 16 * (2 * m + (i >> 2)) + 4 * (l >> 4) + (i & 3);
                    const float w = (row < n_rows ? W[(size_t)row * ld + col] : 0.f) * S;
                    const _Float16 h = (_Float16)w;
                    out[((size_t)((blk * KS + m) * 2 + 0) * 64 + l) * 8 + i] = h;
                    out[((size_t)((blk * KS + m) * 2 + 1) * 64 + l) * 8 + i] = (_Float16)(w - (float)h);
                }
}
// power of two that brings the largest |entry| of W[0..rows)[col0..col0+cols) into [2^13, 2^14)   (1 for an all-zero matrix).
// `bias` (n_bias entries, may be NULL) is the layer's bias row, which the kernel multiplies by the same factor: the factor is capped so
// that S |b| stays <= 2^14 -- a near-zero matrix beside O(1) biases (a pruned or freshly initialised layer) would otherwise scale the
// biases to 1e18 and overflow the LayerNorm's sum of squares; what the cap costs is precision of a product that is negligible beside
// that bias anyway.  phi's first Linear packs only its e half (columns F..2F), but the kernel multiplies the per-atom P = s W_s^T + b0
// by the same factor, so its factor is taken over all 2F columns and b0: S |W_s| <= 2^14 bounds S |P| by 2^14 (|s|_1 + 1).
float matrix_pow2_scale(const float* W, int ld, int rows, int col0, int cols, const float* bias = nullptr, int n_bias = 0)
{
    float mx = 0.f, mb = 0.f;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) mx = std::max(mx, std::fabs(W[(size_t)r * ld + col0 + c]));
    for (int i = 0; i < n_bias; ++i) mb = std::max(mb, std::fabs(bias[i]));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.0f;
    int e; std::frexp(mx, &e);                      // mx = f * 2^e, f in [0.5, 1)
    int k = std::min(60, std::max(-60, 14 - e));
    if (mb > 0.f && std::isfinite(mb)) { int eb; std::frexp(mb, &eb); k = std::min(k, std::max(-60, 14 - eb)); }
    return std::ldexp(1.0f, k);
}

// fp16 storage mode (r16::OpndH): the hi fragments alone, half the bytes:  frag[(blk*(NBK/2) + m)*64 + l][i]
void pack_chunk16_half(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)NBK * 64 * 4);
    _Float16* out = reinterpret_cast<_Float16*>(dst.data() + base);
    const int KS = NBK / 2;
    for (int blk = 0; blk < 2; ++blk)
        for (int m = 0; m < KS; ++m)
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < 8; ++i) {
                    const int row = row0 + 16 * blk + (l & 15), col = col0 + 16 * (2 * m + (i >> 2)) + 4 * (l >> 4) + (i & 3);
                    out[((size_t)(blk * KS + m) * 64 + l) * 8 + i] = (_Float16)(row < n_rows ? W[(size_t)row * ld + col] : 0.f);
                }
}

struct MlpOff { size_t W0, b0, g0, be0, W1, b1, g1, be1, W2, b2; int f_in, f_h, f_out; };
static size_t take_mlp(MlpOff& m, size_t o, int f_in, int f_h, int f_out)
{
    m.f_in = f_in; m.f_h = f_h; m.f_out = f_out;
    m.W0 = o; o += (size_t)f_h * f_in; m.b0 = o; o += f_h; m.g0 = o; o += f_h; m.be0 = o; o += f_h;
    m.W1 = o; o += (size_t)f_h * f_h;  m.b1 = o; o += f_h; m.g1 = o; o += f_h; m.be1 = o; o += f_h;
    m.W2 = o; o += (size_t)f_out * f_h; m.b2 = o; o += f_out;
    return o;
}

template <typename T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;
    void alloc(size_t count) { release(); if (count) { HIP_CHECK(hipMalloc((void**)&p, count * sizeof(T))); n = count; } }
    void upload(const std::vector<T>& h) { alloc(h.size()); if (n) HIP_CHECK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice)); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
    ~DevBuf() { release(); }
};

struct Stream { size_t off4; int nch; };      // offset into the packed buffer in float4 units

}  // namespace ti

using namespace ti;

// ====================================================================================================== handle
struct ti_handle {
    int kind = 0;                 // 0 painn, 1 adw
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
    int NB = 0, nE = 0, ncond = 0, G = 1, nblk = 0;
    MlpOff embed{}, readout{}; std::vector<MlpOff> phi, w, upd; std::vector<size_t> U, V;
    size_t edge_emb = 0, atom_emb = 0, Vr = 0; float b2_gate = 0.f;
    Stream st_embed16{}; std::vector<Stream> st_edge, st_edge1, st_update;      // st_edge1: the message kernel's one-accumulator format (TI_PREC_F16X2)
    // edge templates (ti_internal.hpp): [0] throughput (G molecules per group), [1] latency (G = 1, P parts per molecule);
    // G / P / nblk / rows / slotnode below are those of the ACTIVE one (select_template, once per API call)
    struct Tpl {
        int G = 1, P = 1, nblk = 0;
        DevBuf<uint32_t> rows; DevBuf<int32_t> slotnode;
        std::vector<uint32_t> rows_h;             // host copy of `rows` (masked_rows)
        std::vector<int> part_of, part_start, part_len;     // per sorted edge: its part; per part: first sorted edge, edges
        std::vector<int> pos;                     // row of (molecule-in-group m, sorted edge k) inside its part: pos[m * part_len + (k - part_start)]
        int max_slots = 0;                        // most destination atoms in any row block (<= EDGE_MAX_SLOTS)
    } tpl[3];
    // tpl[2]: the pair-major template (ti_internal.hpp; painn_pair_kernel.hpp), built when the graph is symmetric and the pair kernel
    // exists for this width / precision.  pair_pos[(m * A + src) * A + dst] = e row of that directed edge of molecule-in-group m inside
    // its group: (block * 2 + direction) * 16 + pair row
    bool has_pair = false; std::vector<int> pair_pos; double pair_fill = 0.0;
    DevBuf<int32_t> pair_plist; int pair_kmax = 0;     // per atom of a group: its partial-sum rows (pair_template.hpp)
    DevBuf<float> part;                                // [groups * nblk][8][7 F] partial sums of the pair-major kernel
    int n_tpl = 1, active = 0, parts = 1, max_slots = 0, pinned_tpl = TI_TEMPLATE_AUTO;
    // every atom has incoming edges: the edge kernels' first touch of an accumulator replaces its contents (ti_internal.hpp
    // SLOT_FIRST_TOUCH) and nothing zeroes the accumulators between layers or calls; otherwise the update kernel zeroes them as before
    bool first_touch = false;
    // per-molecule edge sets (ti_painn_set_edge_mask): [emask_B][A] words, in force for calls over emask_B molecules (0: no mask);
    // emask_sym: every molecule's set is symmetric over the template (the pair layout is eligible).  mrows[t]: the row words of
    // template t per (group, part) of those molecules with the absent edges switched off (masked_rows), built on first use.
    std::vector<uint32_t> emask; long long emask_B = 0; bool emask_sym = true;
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

namespace {

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

void set_device(const ti_handle* h) { HIP_CHECK(hipSetDevice(h->device)); }

// ------------------------------------------------------------------------------------------------ painn create
// Packs the rows of `count` molecules' edges with sorted position in [k0, k1) into 16-row blocks: rows keep their (molecule, dst,
// src) order; a block takes at most EDGE_MAX_SLOTS destination atoms (a further one starts the next block, the rest is padding).
// pos[m * (k1 - k0) + (k - k0)] = row of that edge inside the part; returns the number of blocks used.
static int pack_part(const ti_handle* h, const int32_t* dst, int count, int k0, int k1, std::vector<int>& pos)
{
    constexpr int RB = ti::EDGE_ROWS_PER_BLOCK;
    const int per = k1 - k0;
    pos.assign((size_t)count * per, 0);
    int row = 0, nslot = 0, last_key = -1;
    for (int m = 0; m < count; ++m)
        for (int k = k0; k < k1; ++k) {
            const int key = m * 256 + dst[h->perm[k]];
            if (row % RB == 0) { nslot = 0; last_key = -1; }
            if (key != last_key) {
                if (nslot == ti::EDGE_MAX_SLOTS) { row = (row + RB - 1) / RB * RB; nslot = 0; }
                ++nslot; last_key = key;
            }
            pos[(size_t)m * per + (k - k0)] = row++;
        }
    return (row + RB - 1) / RB;
}

// row / slot words of a packed part (ti_internal.hpp); returns the most slots any block holds
static int fill_part(const ti_handle* h, const int32_t* src, const int32_t* dst, const int32_t* etype, int count, int k0, int k1, int nblk,
                     const std::vector<int>& pos, uint32_t* rw, int32_t* sn)
{
    constexpr int RB = ti::EDGE_ROWS_PER_BLOCK;
    const int per = k1 - k0;
    for (int i = 0; i < nblk * RB; ++i) { rw[i] = (uint32_t)63 << 18; sn[i] = -1; }
    std::vector<int> nslot(std::max(nblk, 1), 0), last_key(std::max(nblk, 1), -1);
    std::vector<char> touched((size_t)count * 256, 0);          // rows are visited in increasing order: the first block seen is the first executed
    int most = 0;
    for (int m = 0; m < count; ++m)
        for (int kk = 0; kk < per; ++kk) {
            const int r = pos[(size_t)m * per + kk], blk = r / RB, k = h->perm[k0 + kk];
            const int key = m * 256 + dst[k];
            if (key != last_key[blk]) {
                const int32_t first = (h->first_touch && !touched[key]) ? ti::SLOT_FIRST_TOUCH : 0;
                touched[key] = 1;
                sn[(size_t)blk * RB + nslot[blk]] = first | (m << 8) | dst[k]; ++nslot[blk]; last_key[blk] = key;
            }
            most = std::max(most, nslot[blk]);
            rw[r] = 1u | ((uint32_t)m << 1) | ((uint32_t)src[k] << 6) | ((uint32_t)dst[k] << 11) | ((uint32_t)etype[k] << 16) |
                    ((uint32_t)(nslot[blk] - 1) << 18);
        }
    return most;
}

void build_templates(ti_handle* h, const int32_t* src, const int32_t* dst, const int32_t* etype)
{
    const int A = h->d.n_atoms, E = h->d.n_edges;
    constexpr int RB = ti::EDGE_ROWS_PER_BLOCK;
    {
        std::vector<char> has_in(A, 0);
        for (int k = 0; k < E; ++k) has_in[dst[k]] = 1;
        h->first_touch = E > 0 && std::all_of(has_in.begin(), has_in.end(), [](char c) { return c != 0; });
        // triage switch: TI_ZERO_ACC=1 at creation forces the zeroing path (memsets before an evaluation, the update kernel clears
        // what it consumed, every accumulator update is an add) -- tests/test_gpu_pair.py compares the two paths on poisoned accumulators
        if (const char* z = std::getenv("TI_ZERO_ACC")) if (z[0] == '1') h->first_touch = false;
    }
    h->perm.resize(E);
    for (int k = 0; k < E; ++k) h->perm[k] = k;
    std::stable_sort(h->perm.begin(), h->perm.end(), [&](int a, int b) {
        return dst[a] != dst[b] ? dst[a] < dst[b] : src[a] < src[b];
    });
    // ---- throughput template: smallest G in 1..8 whose padding waste is <= 2 %, else the least wasteful
    {
        int bestG = 1; double bestW = 2.0;
        std::vector<int> pos;
        for (int G = 1; G <= 8 && E > 0; ++G) {
            const int rows = G * E, padded = pack_part(h, dst, G, 0, E, pos) * RB;
            const double waste = double(padded - rows) / padded;
            if (waste < bestW - 1e-12) { bestW = waste; bestG = G; }
            if (waste <= 0.02) { bestG = G; break; }
        }
        ti_handle::Tpl& T = h->tpl[0];
        T.G = bestG; T.P = 1;
        T.nblk = E > 0 ? pack_part(h, dst, bestG, 0, E, T.pos) : 0;
        T.part_of.assign(E, 0); T.part_start.assign(1, 0); T.part_len.assign(1, E);
        std::vector<uint32_t> rw((size_t)std::max(T.nblk, 1) * RB); std::vector<int32_t> sn(rw.size());
        T.max_slots = fill_part(h, src, dst, etype, bestG, 0, E, T.nblk, T.pos, rw.data(), sn.data());
        if (T.nblk == 0) { rw[0] = (uint32_t)63 << 18; sn[0] = -1; }
        T.rows.upload(rw); T.slotnode.upload(sn); T.rows_h = rw;
    }
    // ---- latency template: one molecule per group, its destination atoms cut into P ranges of near-equal row count; the
    // largest P <= 8 whose padding waste stays <= 15 % (parts need whole row blocks).  Built only if it offers more waves.
    h->n_tpl = 1;
    if (E >= 2 * RB) {
        std::vector<int> first_of(A + 1, E);           // first sorted edge with destination >= a
        for (int k = E - 1; k >= 0; --k) first_of[dst[h->perm[k]]] = k;
        for (int a = A - 1; a >= 0; --a) first_of[a] = std::min(first_of[a], first_of[a + 1]);
        std::vector<int> pos;
        int bestP = 1, best_nblk = pack_part(h, dst, 1, 0, E, pos); std::vector<int> best_cut{0, E};
        for (int P = 2; P <= 8; ++P) {
            std::vector<int> cut{0};
            for (int q = 1; q < P; ++q) {             // atom boundary closest to q/P of the rows
                const int want = (int)((long long)E * q / P);
                int bk = cut.back();
                for (int a = 0; a <= A; ++a) if (first_of[a] > cut.back() && std::abs(first_of[a] - want) < std::abs(bk - want)) bk = first_of[a];
                if (bk <= cut.back()) { cut.clear(); break; }
                cut.push_back(bk);
            }
            if (cut.empty() || cut.back() >= E) continue;
            cut.push_back(E);
            int nblk = 0;
            for (int q = 0; q < P; ++q) nblk = std::max(nblk, pack_part(h, dst, 1, cut[q], cut[q + 1], pos));
            if (double(P * nblk * RB - E) / (P * nblk * RB) <= 0.15) { bestP = P; best_nblk = nblk; best_cut = cut; }
        }
        if (bestP * h->tpl[0].G > 1) {
            ti_handle::Tpl& T = h->tpl[1];
            T.G = 1; T.P = bestP; T.nblk = best_nblk; T.max_slots = 0;
            T.part_start.assign(best_cut.begin(), best_cut.end() - 1);
            T.part_of.resize(E); T.part_len.resize(bestP); T.pos.assign(E, 0);
            for (int q = 0; q < bestP; ++q) for (int k = best_cut[q]; k < best_cut[q + 1]; ++k) T.part_of[k] = q;
            std::vector<uint32_t> rw((size_t)bestP * best_nblk * RB); std::vector<int32_t> sn(rw.size());
            for (int q = 0; q < bestP; ++q) {
                T.part_len[q] = best_cut[q + 1] - best_cut[q];
                pack_part(h, dst, 1, best_cut[q], best_cut[q + 1], pos);
                std::copy(pos.begin(), pos.end(), T.pos.begin() + best_cut[q]);
                T.max_slots = std::max(T.max_slots, fill_part(h, src, dst, etype, 1, best_cut[q], best_cut[q + 1], best_nblk, pos,
                                                              rw.data() + (size_t)q * best_nblk * RB, sn.data() + (size_t)q * best_nblk * RB));
            }
            T.rows.upload(rw); T.slotnode.upload(sn); T.rows_h = rw;
            h->n_tpl = 2;
        }
    }
    h->esrc.assign(src, src + E); h->edst.assign(dst, dst + E);
}


// ---- pair-major template: pair_template.hpp builds it (pure host code, unit-tested on the CPU); this uploads it
static bool build_pair_template(ti_handle* h, const int32_t* src, const int32_t* dst, const int32_t* etype)
{
    ti::PairTemplate pt;
    if (!ti::build_pair_template(h->d.n_atoms, h->d.n_edges, src, dst, etype, pt, h->first_touch && !pair_uses_partials())) return false;
    ti_handle::Tpl& T = h->tpl[2];
    T.G = pt.G; T.P = 1; T.nblk = pt.nblk; T.max_slots = 4;
    T.rows.upload(pt.rows); T.slotnode.upload(pt.slotnode); T.rows_h = pt.rows;
    h->pair_pos = pt.pair_pos; h->pair_fill = pt.fill;
    h->pair_plist.upload(pt.plist); h->pair_kmax = pt.kmax;
    return true;
}

// The layout the handle is pinned to (ti_painn_set_template, or TI_TEMPLATE in the environment), TI_TEMPLATE_AUTO if none.
int pinned_template(const ti_handle* h)
{
    int want = h->pinned_tpl;
    if (const char* e = std::getenv("TI_TEMPLATE"))
        want = std::strcmp(e, "latency") == 0 ? 1 : std::strcmp(e, "throughput") == 0 ? 0 : std::strcmp(e, "pair") == 0 ? 2 : want;
    return want;
}
// an edge mask is in force whose molecules' sets are not all symmetric: the pair rows (one w factor for both directions) cannot take it
bool mask_blocks_pair(const ti_handle* h) { return h->emask_B > 0 && !h->emask_sym; }

// Template for a call over B molecules: the latency template while the throughput one would leave SIMDs without a wave
// (fewer groups than the 1024 SIMDs of the chip); TI_TEMPLATE=throughput|latency pins it (tests, reproducibility across shards).
int template_for(const ti_handle* h, long long B, bool allow_pair = true)
{
    int dir_pick = 0;                        // among the directed layouts: latency while the throughput one would leave SIMDs idle
    if (h->n_tpl > 1) dir_pick = (B + h->tpl[0].G - 1) / h->tpl[0].G < 1024 ? 1 : 0;
    const bool pair_ok = h->has_pair && allow_pair && !mask_blocks_pair(h);
    // pair-major rows once they fill the chip (one wave per group of G molecules) and cost less than the directed rows: a pair block
    // runs 84 chunk products for 16 pairs where a directed block runs 56 for 16 edges, at half the weight-chunk visits per edge
    int pick = dir_pick;
    if (pair_ok) {
        const ti_handle::Tpl &T = h->tpl[2], &D = h->tpl[0];
        if ((B + T.G - 1) / T.G >= 1024 && 1.5 * T.nblk / T.G <= (double)D.nblk / D.G) pick = 2;
    }
    const int want = pinned_template(h);
    if (want == TI_TEMPLATE_THROUGHPUT) pick = 0;
    else if (want == TI_TEMPLATE_LATENCY) pick = h->n_tpl > 1 ? 1 : 0;
    else if (want == TI_TEMPLATE_PAIR) pick = pair_ok ? 2 : dir_pick;
    return pick;
}

// allow_pair = false: the divergence / tangent entry points (their kernels walk directed rows)
void select_template(ti_handle* h, long long B, bool allow_pair = true)
{
    if (h->emask_B > 0 && B != h->emask_B)
        throw std::invalid_argument("the edge mask in force is for " + std::to_string(h->emask_B) + " molecules, the call has " + std::to_string(B));
    if (allow_pair && h->has_pair && mask_blocks_pair(h) && pinned_template(h) == TI_TEMPLATE_PAIR)
        throw Unsupported("the pair layout is pinned, and the edge mask in force is not symmetric for every molecule");
    const int pick = template_for(h, B, allow_pair);
    const ti_handle::Tpl& T = h->tpl[pick];
    h->active = pick; h->G = T.G; h->parts = T.P; h->nblk = T.nblk; h->rows.p = T.rows.p; h->slotnode.p = T.slotnode.p;
    h->max_slots = T.max_slots;
}

// Row words of template t for the emask_B molecules of the edge mask, per (group, part) -- [groups][P][nblk * 16] -- with every edge
// absent from its molecule (every edge of a pad atom among them: set_graph_state cleared their bits) switched off: slot 63 in directed rows (weight 0 in the per-atom sums, like padding), the valid bit cleared
// in pair rows (w factor 0).  The masked twins of the message kernels read these instead of the template's shared rows.
const uint32_t* masked_rows(ti_handle* h, int t)
{
    if (h->mrows_ok[t]) return h->mrows[t].p;
    const ti_handle::Tpl& T = h->tpl[t];
    const long long B = h->emask_B, groups = (B + T.G - 1) / T.G;
    const int A = h->d.n_atoms;
    const size_t per = (size_t)T.nblk * ti::EDGE_ROWS_PER_BLOCK;
    std::vector<uint32_t> out((size_t)groups * T.P * per);
    const uint32_t* m = h->emask.data();
    const uint8_t* pt = h->ptype.empty() ? nullptr : h->ptype.data();      // per-molecule edge types of the present rows (ti_painn_set_molecules)
    for (long long g = 0; g < groups; ++g)
        for (int part = 0; part < T.P; ++part) {
            const uint32_t* src = T.rows_h.data() + (size_t)part * per;
            uint32_t* dst = out.data() + ((size_t)g * T.P + part) * per;
            for (size_t i = 0; i < per; ++i) {
                uint32_t w = src[i];
                if (w & 1u) {
                    if (t == 2) {
                        const long long mol = g * T.G + ti::prow_molI(w);
                        if (mol < B && !((m[mol * A + ti::prow_atomJ(w)] >> ti::prow_atomI(w)) & 1u)) w &= ~1u;
                        else if (mol < B && pt) w = (w & ~(3u << 17)) | ((uint32_t)pt[((size_t)mol * A + ti::prow_atomI(w)) * A + ti::prow_atomJ(w)] << 17);
                    } else {
                        const long long mol = g * T.G + ti::row_mol(w);
                        if (mol < B && !((m[mol * A + ti::row_dst(w)] >> ti::row_src(w)) & 1u)) w |= 63u << 18;
                        else if (mol < B && pt) w = (w & ~(3u << 16)) | ((uint32_t)pt[((size_t)mol * A + ti::row_src(w)) * A + ti::row_dst(w)] << 16);
                    }
                }
                dst[i] = w;
            }
        }
    h->mrows[t].upload(out);
    h->mrows_ok[t] = true;
    return h->mrows[t].p;
}

// row of (molecule m, sorted edge k) in the e / te layout of the active template
size_t edge_row_of(const ti_handle* h, size_t m, size_t k)
{
    const ti_handle::Tpl& T = h->tpl[h->active];
    if (h->active == 2) {                   // pair-major rows: [group][block][direction][16]
        const size_t A = h->d.n_atoms;
        return (m / T.G) * (size_t)T.nblk * 2 * ti::EDGE_ROWS_PER_BLOCK + (size_t)h->pair_pos[((m % T.G) * A + h->esrc[h->perm[k]]) * A + h->edst[h->perm[k]]];
    }
    // throughput template: one part, pos over (molecule in group, sorted edge); latency template: G = 1, pos over the sorted edge
    const size_t part = T.part_of[k], r = T.pos[(m % T.G) * (size_t)h->d.n_edges + k];
    return ((m / T.G) * T.P + part) * T.nblk * ti::EDGE_ROWS_PER_BLOCK + r;
}

// edge rows (e, te) per molecule-group slot, the larger of the two templates: rows a batch of B molecules needs
size_t edge_rows_for(const ti_handle* h, long long B, long long copies = 1)
{
    size_t best = 1;
    for (int t = 0; t < h->n_tpl; ++t) {
        const ti_handle::Tpl& T = h->tpl[t];
        best = std::max<size_t>(best, (size_t)((B + T.G - 1) / T.G) * (size_t)copies * T.P * T.nblk * ti::EDGE_ROWS_PER_BLOCK);
    }
    if (h->has_pair && copies == 1)         // two directions per pair row
        best = std::max<size_t>(best, (size_t)((B + h->tpl[2].G - 1) / h->tpl[2].G) * h->tpl[2].nblk * 2 * ti::EDGE_ROWS_PER_BLOCK);
    return best;
}

void pack_painn(ti_handle* h, const float* wts)
{
    const int F = h->d.n_features, L = h->d.n_layers, NB = h->NB, nE = h->nE;
    std::vector<float> pk;
    auto begin_stream = [&]() { return pk.size() / 4; };
    size_t o = 0;
    const int NBK = F / 16;
    const int prec = h->d.precision;          // 16-row chunks: f32 image, (hi, lo) fp16 image of the same size, or hi-only fp16 image of half the size
    const size_t ch4 = (prec == TI_PREC_F16 ? 128 : 256) * (size_t)NB;      // float4 per 16-row chunk
    auto chunk16 = [&](size_t W, int ld, int n_rows, int row0, int col0) {
        if (prec == TI_PREC_F16) pack_chunk16_half(pk, wts + W, ld, n_rows, row0, col0, NBK);
        else if (prec == TI_PREC_F16X2) pack_chunk16_split(pk, wts + W, ld, n_rows, row0, col0, NBK);
        else pack_chunk16(pk, wts + W, ld, n_rows, row0, col0, NBK);
    };
    auto layer16 = [&](size_t W, int ld, int n_rows, int col0) { for (int nbo = 0; nbo < NB; ++nbo) chunk16(W, ld, n_rows, 32 * nbo, col0); };
    auto end_stream16 = [&](size_t off4) { return Stream{off4, (int)((pk.size() / 4 - off4) / ch4)}; };
    auto pad_even = [&](size_t off4) { if (((pk.size() / 4 - off4) / ch4) % 2) pk.resize(pk.size() + 4 * ch4, 0.f); };
    o = begin_stream();                              // embed kernel, 16-row chunk format: L1 by input segment, L2, L3, then P for the first message block
    for (int seg = 0; seg < nE; ++seg) layer16(h->embed.W0, nE * F, F, seg * F);
    layer16(h->embed.W1, F, F, 0); layer16(h->embed.W2, F, F, 0);
    if (L > 0) layer16(h->phi[0].W0, 2 * F, F, 0);
    else pk.resize(pk.size() + 4 * ch4 * NB, 0.f);
    pad_even(o);
    h->st_embed16 = end_stream16(o);
    for (int l = 0; l < L; ++l) {
        const bool first = l == 0, last = l == L - 1;
        o = begin_stream();                          // edge kernel: 16-row chunk format
        layer16(h->w[l].W0, F, F, 0); layer16(h->w[l].W1, F, F, 0);
        layer16(h->phi[l].W0, 2 * F, F, F);        // the e half of [s[src] | e]
        layer16(h->phi[l].W1, F, F, 0);
        for (int nbo = 0; nbo < NB; ++nbo)
            for (int c : {2, 3, 1, 0, 4}) {       // consumption order of painn_edge_kernel: ds, de, sed, gates, cross gates
                if (c == 3 && last) continue;
                if ((c == 0 || c == 4) && first) continue;
                chunk16(h->phi[l].W2, F, 5 * F, c * F + 32 * nbo, 0);
                chunk16(h->w[l].W2, F, 5 * F, c * F + 32 * nbo, 0);
            }
        h->st_edge.push_back(end_stream16(o));
        if (edge_uses_one_chain(NB, prec)) {         // the same chunks in the one-accumulator format, each matrix scaled by its own power of two
            const float S[6] = {matrix_pow2_scale(wts + h->w[l].W0, F, F, 0, F, wts + h->w[l].b0, F), matrix_pow2_scale(wts + h->w[l].W1, F, F, 0, F, wts + h->w[l].b1, F),
                                matrix_pow2_scale(wts + h->phi[l].W0, 2 * F, F, 0, 2 * F, wts + h->phi[l].b0, F), matrix_pow2_scale(wts + h->phi[l].W1, F, F, 0, F, wts + h->phi[l].b1, F),
                                matrix_pow2_scale(wts + h->phi[l].W2, F, 5 * F, 0, F, wts + h->phi[l].b2, 5 * F), matrix_pow2_scale(wts + h->w[l].W2, F, 5 * F, 0, F, wts + h->w[l].b2, 5 * F)};
            auto layer1 = [&](size_t W, int ld, int n_rows, int col0, float sc) { for (int nbo = 0; nbo < NB; ++nbo) pack_chunk16_split1(pk, wts + W, ld, n_rows, 32 * nbo, col0, NBK, sc); };
            o = begin_stream();
            layer1(h->w[l].W0, F, F, 0, S[0]); layer1(h->w[l].W1, F, F, 0, S[1]);
            layer1(h->phi[l].W0, 2 * F, F, F, S[2]);
            layer1(h->phi[l].W1, F, F, 0, S[3]);
            for (int nbo = 0; nbo < NB; ++nbo)
                for (int c : {2, 3, 1, 0, 4}) {
                    if (c == 3 && last) continue;
                    if ((c == 0 || c == 4) && first) continue;
                    pack_chunk16_split1(pk, wts + h->phi[l].W2, F, 5 * F, c * F + 32 * nbo, 0, NBK, S[4]);
                    pack_chunk16_split1(pk, wts + h->w[l].W2, F, 5 * F, c * F + 32 * nbo, 0, NBK, S[5]);
                }
            h->st_edge1.push_back(end_stream16(o));
            h->edge_scale.insert(h->edge_scale.end(), S, S + 6);
        }
        o = begin_stream();                          // update kernel: 16-row chunk format, order of painn_update_kernel
        layer16(h->V[l], F, F, 0);                                                    // phase A (3 components per visit)
        layer16(h->upd[l].W0, 2 * F, F, 0); layer16(h->upd[l].W0, 2 * F, F, F);      // MLP L1: |vv| part, s part
        layer16(h->upd[l].W1, F, F, 0);
        for (int nbo = 0; nbo < NB; ++nbo) {
            chunk16(h->upd[l].W2, F, 3 * F, F + 32 * nbo, 0);                         // scale_squared_norm
            chunk16(h->upd[l].W2, F, 3 * F, 2 * F + 32 * nbo, 0);                     // add_invariant_features
        }
        layer16(h->upd[l].W2, F, 3 * F, 0);                                           // gates
        for (int c = 0; c < 3; ++c) layer16(h->U[l], F, F, 0);                        // phase C (one spatial component per walk)
        if (!last) layer16(h->phi[l + 1].W0, 2 * F, F, 0);                            // phase D
        pad_even(o);                                                                  // whole superchunks
        h->st_update.push_back(end_stream16(o));
        // tangent edge kernel (painn_jvp_kernels.hip): the phi branch's chunks in the consumption order of the edge kernels
        for (int which = 1; which < 2; ++which) {      // the phi branch alone (the primal pass reads the primal edge stream)
            const MlpOff& m = h->phi[l];
            o = begin_stream();
            layer16(m.W0, 2 * F, F, F);
            layer16(m.W1, F, F, 0);
            for (int nbo = 0; nbo < NB; ++nbo)
                for (int c : {2, 3, 1, 0, 4}) {
                    if (c == 3 && last) continue;
                    if ((c == 0 || c == 4) && first) continue;
                    chunk16(m.W2, F, 5 * F, c * F + 32 * nbo, 0);
                }
            const int real = end_stream16(o).nch;   // an odd count gets one pad chunk, which the kernels swallow once per row block
            pad_even(o);
            h->st_jvp_phi.push_back(end_stream16(o));
            h->jvp_phi_pad.push_back(real & 1);
        }
        o = begin_stream();                          // tangent update kernel: same order, V and U once per spatial component
        for (int c = 0; c < 3; ++c) layer16(h->V[l], F, F, 0);
        layer16(h->upd[l].W0, 2 * F, F, 0); layer16(h->upd[l].W0, 2 * F, F, F);
        layer16(h->upd[l].W1, F, F, 0);
        for (int nbo = 0; nbo < NB; ++nbo) {
            chunk16(h->upd[l].W2, F, 3 * F, F + 32 * nbo, 0);
            chunk16(h->upd[l].W2, F, 3 * F, 2 * F + 32 * nbo, 0);
        }
        layer16(h->upd[l].W2, F, 3 * F, 0);
        for (int c = 0; c < 3; ++c) layer16(h->U[l], F, F, 0);
        if (!last) layer16(h->phi[l + 1].W0, 2 * F, F, 0);
        pad_even(o);
        h->st_jvp_update.push_back(end_stream16(o));
    }
    // readout kernels (primal and tangent): 16-row chunk format
    o = begin_stream();
    for (size_t Wm : {h->readout.W0, h->readout.W1})
        for (int nbo = 0; nbo < NB; ++nbo) {
            chunk16(Wm, F, F, 32 * nbo, 0);
        }
    pad_even(o);
    h->st_jvp_readout = end_stream16(o);
    h->packed.upload(pk);
    {
        std::vector<float> rv;                       // order = struct RV in painn_jvp_kernels.hip
        const MlpOff& r = h->readout;
        // Vr follows the 2-float readout bias in the canonical layout (h->Vr itself points at an aligned copy inside `flat`)
        for (size_t off : {r.b0, r.g0, r.be0, r.b1, r.g1, r.be1, r.W2 + (size_t)F, r.b2 + 2}) rv.insert(rv.end(), wts + off, wts + off + F);
        h->jvp_ro_vecs.upload(rv);
    }
    // per-layer vector block of the edge kernel (order = struct EV in painn_kernels.hip)
    std::vector<float> ev;
    for (int l = 0; l < L; ++l) {
        const MlpOff &w = h->w[l], &ph = h->phi[l];
        for (size_t off : {w.b0, w.g0, w.be0, w.b1, w.g1, w.be1, ph.g0, ph.be0, ph.b1, ph.g1, ph.be1}) ev.insert(ev.end(), wts + off, wts + off + F);
        ev.insert(ev.end(), wts + ph.b2, wts + ph.b2 + 5 * F);
        ev.insert(ev.end(), wts + w.b2, wts + w.b2 + 5 * F);
    }
    h->edge_vecs.upload(ev);
    if (edge_uses_one_chain(NB, prec)) {             // the message kernel's copy: bias rows times the scale of their matrix (EV order: W_B0 = 0, W_B1 = 3, P_B1 = 8, P_B2 = 11..15, W_B2 = 16..20)
        std::vector<float> ev1 = ev;
        for (int l = 0; l < L; ++l) {
            const float* S = h->edge_scale.data() + (size_t)l * 6;
            float* b = ev1.data() + (size_t)l * 21 * F;
            auto mul = [&](int row, int n, float sc) { for (int i = 0; i < n * F; ++i) b[(size_t)row * F + i] *= sc; };
            mul(0, 1, S[0]); mul(3, 1, S[1]); mul(8, 1, S[3]); mul(11, 5, S[4]); mul(16, 5, S[5]);
        }
        h->edge_vecs1.upload(ev1);
    }
    std::vector<float> uv;                           // order = struct UV in painn_kernels.hip
    for (int l = 0; l < L; ++l) {
        const MlpOff& u = h->upd[l];
        for (size_t off : {u.b0, u.g0, u.be0, u.b1, u.g1, u.be1}) uv.insert(uv.end(), wts + off, wts + off + F);
        uv.insert(uv.end(), wts + u.b2, wts + u.b2 + 3 * F);
        if (l + 1 < L) uv.insert(uv.end(), wts + h->phi[l + 1].b0, wts + h->phi[l + 1].b0 + F);
        else uv.insert(uv.end(), F, 0.f);
    }
    h->upd_vecs.upload(uv);
}

void ensure_painn_ws(ti_handle* h, long long B)
{
    if (B <= h->cap) return;
    const size_t A = h->d.n_atoms, F = h->d.n_features, N = (size_t)B * A;
    h->x.alloc(N * 3); h->b1.alloc(N * 3); h->b2.alloc(N * 3); h->xt.alloc(N * 3);
    h->cond.alloc(std::max<size_t>(N * h->ncond, 1));
    const size_t se = h->d.precision == TI_PREC_F16 ? 2 : 1;      // state tensors s, P, v, e: fp16 in the storage mode (2 per float slot)
    h->s.alloc((N * F + se - 1) / se); h->P.alloc((N * F + se - 1) / se);
    h->v.alloc((N * 3 * F + se - 1) / se); h->dvacc.alloc(N * 3 * F); h->cacc.alloc(N * 3 * F); h->dsacc.alloc(N * F);
    h->e.alloc((edge_rows_for(h, B) * F + se - 1) / se);
    // parked geometry of a drift evaluation (painn_edge_kernel.hpp): the encoding operand of every edge row (as many bytes as e) and edge_dir
    h->enc.alloc((edge_rows_for(h, B) * F + se - 1) / se); h->geo.alloc(edge_rows_for(h, B) * 4);
    h->divb.alloc(B); h->div2.alloc(B); h->dl.alloc(B); h->dlscaled.alloc(B);
    if (h->has_pair && pair_uses_partials()) h->part.alloc((size_t)((B + h->tpl[2].G - 1) / h->tpl[2].G) * h->tpl[2].nblk * 8 * 7 * F);
    h->cap = B;
}

// ---- forward-mode derivative: tangent workspace over ceil(B/G)*D*G virtual molecules (painn_jvp_kernels.hip header)
long long jvp_virtual_molecules(const ti_handle* h, long long B, int D) { return (B + h->G - 1) / h->G * D * h->G; }

size_t jvp_bytes_per_vm(const ti_handle* h)
{
    const size_t A = h->d.n_atoms, F = h->d.n_features;
    const size_t erows = ((size_t)h->parts * h->nblk * ti::EDGE_ROWS_PER_BLOCK + h->G - 1) / h->G;
    return (A * F * 12 + erows * F + A * 3) * sizeof(float);
}

void ensure_jvp_ws(ti_handle* h, long long B, int D)
{
    const long long VB = jvp_virtual_molecules(h, B, D);
    const size_t A = h->d.n_atoms, F = h->d.n_features, N = (size_t)VB * A;
    const size_t pgroups = ((size_t)B + h->G - 1) / h->G * h->parts;
    const size_t wq_floats = std::max<size_t>(pgroups * h->nblk * 5 * h->NB * 6 * 64 * 4, 4);
    const size_t st_floats = std::max<size_t>(pgroups * h->nblk * 4 * (2 * h->NB) * 64 * 4, 4);
    if (h->wq.n < wq_floats) h->wq.alloc(wq_floats);
    if (h->phist.n < st_floats) h->phist.alloc(st_floats);
    const size_t ns_floats = (((size_t)B * A + 15) / 16) * 13 * (2 * h->NB) * 64 * 4;
    if (h->nodest.n < ns_floats) h->nodest.alloc(ns_floats);
    const size_t te_floats = (size_t)VB / h->G * h->parts * h->nblk * ti::EDGE_ROWS_PER_BLOCK * F;
    if (h->te.n < te_floats) h->te.alloc(std::max<size_t>(te_floats, 1));
    if (VB <= h->jvp_cap) return;
    if (N >= ((size_t)1 << 31)) throw std::invalid_argument("too many tangent nodes in one pass (lower TI_JVP_WS_GB)");
    h->ts.alloc(N * F); h->tP.alloc(N * F); h->tdsacc.alloc(N * F);
    h->tv.alloc(N * 3 * F); h->tdvacc.alloc(N * 3 * F); h->tcacc.alloc(N * 3 * F);
    h->tout.alloc(N * 3);
    h->jvp_cap = VB;
}

// molecules per tangent pass with D directions each, from the HBM budget TI_JVP_WS_GB (default 48 GB of tangent state)
long long jvp_chunk_molecules(const ti_handle* h, int D)
{
    double gb = 48.0;
    if (const char* e = std::getenv("TI_JVP_WS_GB")) gb = std::max(0.001, std::atof(e));
    const double per_mol = (double)jvp_bytes_per_vm(h) * D;
    const long long by_mem = (long long)(gb * 1e9 / per_mol);
    const long long by_index = (long long)(((size_t)1 << 31) - 1) / ((long long)D * h->d.n_atoms) - h->G;
    const long long c = std::max<long long>(1, std::min(by_mem, by_index));
    return c >= h->G ? c / h->G * h->G : c;                  // whole primal groups per pass
}

struct JvpRun {            // one tangent pass riding on a drift evaluation
    int D;                 // seed directions per molecule
    const float* xdot;     // D explicit directions [B][D][A][3] (device; D = 1: ti_painn_drift_jvp, D = k: Hutchinson probes); NULL: unit seeds, D = 3A
    float* tout;           // [B*D*A*3] tangent of the drift (device)
};

// one drift evaluation, everything on h->stream; x_dev / out_dev are device pointers [B*A*3].  With `jr` the tangent
// kernels run in lock step: each reads the primal state its layer's primal kernel is about to overwrite.
// tv (device, [B], may be NULL): one time per molecule instead of t (the embed kernel's per-molecule instantiation).
// b0: the call's first molecule of this batch (the divergence passes run the call in chunks): the edge mask rows it starts at.
void painn_drift_dev(ti_handle* h, const float* x_dev, float t, const float* cond_dev, long long B, float* out_dev,
                     const JvpRun* jr = nullptr, const float* tv = nullptr, long long b0 = 0)
{
    const int A = h->d.n_atoms, F = h->d.n_features, L = h->d.n_layers, NB = h->NB;
    const long long N = B * A, groups = (B + h->G - 1) / h->G * h->parts;         // edge-kernel waves: (molecule group, part)
    hipStream_t st = h->stream;
    const bool split = h->d.precision == TI_PREC_F16X2;
    const int prec = h->d.precision;
    const uint32_t* mrows = nullptr;          // edge mask in force: the masked twins of the message kernels, on per-group row words
    if (h->emask_B > 0) {
        if (b0 % h->G) throw std::invalid_argument("an edge mask needs whole molecule groups per tangent pass (raise TI_JVP_WS_GB)");
        mrows = masked_rows(h, h->active) + (size_t)(b0 / h->G) * h->parts * h->nblk * ti::EDGE_ROWS_PER_BLOCK;
    }
    if (jr && prec == TI_PREC_F16) throw std::invalid_argument("the fp16 storage mode has no divergence / tangent path (use f32 or f16x2)");
    if (jr && h->active == 2) throw std::logic_error("tangent passes walk directed edge rows (select_template(.., allow_pair = false))");
    // mixed species: the kernels below never see what the caller left in pad atoms.  They read copies in which every pad atom is
    // parked beside its molecule's atom 0 (distinct, finite places: an off row's 0 * value stays 0) with cond 0 and direction 0.
    const int32_t* nat = h->ragged ? h->natoms_dev.p + b0 : nullptr;
    const float* xdot = jr ? jr->xdot : nullptr;
    if (nat) {
        const size_t n3 = (size_t)B * A * 3, nc = (size_t)B * A * h->ncond;
        if (h->xpark.n < n3) h->xpark.alloc(n3);
        HIP_CHECK(launch_park_pads(h->xpark.p, x_dev, nat, B, 1, A, 3, 1, st));
        x_dev = h->xpark.p;
        if (nc) {
            if (h->cpark.n < nc) h->cpark.alloc(nc);
            HIP_CHECK(launch_park_pads(h->cpark.p, cond_dev, nat, B, 1, A, h->ncond, 0, st));
            cond_dev = h->cpark.p;
        }
        if (xdot) {
            if (h->dpark.n < n3 * jr->D) h->dpark.alloc(n3 * jr->D);
            HIP_CHECK(launch_park_pads(h->dpark.p, xdot, nat, B * jr->D, jr->D, A, 3, 0, st));
            xdot = h->dpark.p;
        }
    }
    const long long VB = jr ? jvp_virtual_molecules(h, B, jr->D) : 0, VN = VB * A, vgroups = VB / h->G * h->parts;
    if (jr) {
        ensure_jvp_ws(h, B, jr->D);
        h->last_VB = B * jr->D; h->last_D = jr->D;
        const size_t nb = (size_t)VN * F * sizeof(float);
        HIP_CHECK(hipMemsetAsync(h->ts.p, 0, nb, st)); HIP_CHECK(hipMemsetAsync(h->tP.p, 0, nb, st));
        HIP_CHECK(hipMemsetAsync(h->tdsacc.p, 0, nb, st));
        HIP_CHECK(hipMemsetAsync(h->tv.p, 0, 3 * nb, st)); HIP_CHECK(hipMemsetAsync(h->tdvacc.p, 0, 3 * nb, st));
        HIP_CHECK(hipMemsetAsync(h->tcacc.p, 0, 3 * nb, st));
    }
    const size_t vbytes = (size_t)N * 3 * F * sizeof(float);
    // With first-touch accumulators (every atom has incoming edges) nothing needs zeroing: layer 0's edge kernel replaces dsacc and
    // dvacc, its update kernel does not read v and cacc (zero by definition), every later layer replaces all three.  The forward-mode
    // passes read the primal v and cacc of layer 0 themselves, and with no layers the readout reads v: then they are cleared.
    const bool ft = h->first_touch && h->tap < 0;      // (the debug taps read "state + pending accumulators": they want them zeroed after use)
    if (!ft || jr || L == 0) {
        HIP_CHECK(hipMemsetAsync(h->v.p, 0, prec == TI_PREC_F16 ? vbytes / 2 : vbytes, st));
        HIP_CHECK(hipMemsetAsync(h->cacc.p, 0, vbytes, st));
    }
    if (!ft) {
        HIP_CHECK(hipMemsetAsync(h->dvacc.p, 0, vbytes, st));
        HIP_CHECK(hipMemsetAsync(h->dsacc.p, 0, (size_t)N * F * sizeof(float), st));
    }
    {
        EmbedParams p{};
        p.stream = h->S(h->st_embed16); p.nch = h->st_embed16.nch; p.mlp = h->vec(h->embed);
        p.pb0 = L > 0 ? h->F(h->phi[0].b0) : h->F(h->embed.b2);
        p.atom_emb = h->F(h->atom_emb); p.atom_ids = h->atom_ids.p; p.cond = cond_dev; p.ncond = h->ncond; p.A = A; p.N = N;
        p.t = t; p.tv = tv; p.temp_length = h->d.temp_length; p.time_length = h->d.time_length; p.temp_mean = h->d.temp_mean; p.temp_range = h->d.temp_range;
        p.s = h->s.p; p.P = h->P.p;
        Timed tm(h, TI_KERNEL_PAINN_EMBED);
        HIP_CHECK(launch_embed(NB, h->nE, prec, p, st));
    }
    h->last_B = B;
    if (h->tap == 0) return;
    for (int l = 0; l < L; ++l) {
        if (jr && h->nblk > 0) {
            {
                JvpFilterParams p{};
                p.stream = h->S(h->st_edge[l]); p.nch = h->st_edge[l].nch; p.vecs = h->edge_vecs.p + (size_t)l * 21 * F;
                p.edge_emb = h->F(h->edge_emb); p.rows = h->rows.p; p.nblk = h->nblk; p.G = h->G; p.parts = h->parts; p.A = A; p.first = l == 0; p.last = l == L - 1;
                p.B = B; p.n_groups = groups; p.length_scale = h->d.length_scale; p.x = x_dev; p.P = h->P.p; p.e = h->e.p;
                p.wq = reinterpret_cast<float4*>(h->wq.p); p.st = reinterpret_cast<float4*>(h->phist.p);
                const bool typed = mrows && !h->ptype.empty();      // per-molecule edge types: the filter pass reads them from the row words
                if (typed) p.rows = mrows;
                Timed tm(h, TI_KERNEL_PAINN_JVP_FILTER);
                HIP_CHECK(launch_jvp_filter(NB, split, p, st, typed));
            }
            JvpEdgeParams p{};
            p.stream = h->S(h->st_jvp_phi[l]); p.nch = h->st_jvp_phi[l].nch; p.pad = h->jvp_phi_pad[l]; p.vecs = h->edge_vecs.p + (size_t)l * 21 * F;
            p.edge_emb = h->F(h->edge_emb); p.rows = h->rows.p; p.slotnode = h->slotnode.p;
            p.nblk = h->nblk; p.G = h->G; p.parts = h->parts; p.A = A; p.D = jr->D; p.first = l == 0; p.last = l == L - 1;
            p.B = B; p.n_groups = vgroups;
            p.x = x_dev; p.xdot = xdot; p.P = h->P.p; p.v = h->v.p; p.e = h->e.p; p.wq = reinterpret_cast<const float4*>(h->wq.p);
            p.st = reinterpret_cast<const float4*>(h->phist.p); p.tP = h->tP.p; p.tv = h->tv.p;
            p.te = h->te.p; p.tdsacc = h->tdsacc.p; p.tdvacc = h->tdvacc.p; p.tcacc = h->tcacc.p;
            if (mrows) p.rows = mrows;
            Timed tm(h, TI_KERNEL_PAINN_JVP_EDGE);
            HIP_CHECK(launch_jvp_edge(NB, split, p, st, mrows != nullptr));
        }
        if (h->nblk > 0) {
            EdgeParams p{};
            p.stream = h->S(h->st_edge[l]); p.nch = h->st_edge[l].nch; p.vecs = h->edge_vecs.p + (size_t)l * 21 * F;
            p.edge_emb = h->F(h->edge_emb); p.rows = h->rows.p; p.slotnode = h->slotnode.p; p.nslots = nullptr;
            p.nblk = h->nblk; p.G = h->G; p.parts = h->parts; p.A = A; p.max_slots = h->max_slots; p.B = B; p.n_groups = groups; p.length_scale = h->d.length_scale;
            p.x = x_dev; p.P = h->P.p; p.v = h->v.p; p.dsacc = h->dsacc.p; p.dvacc = h->dvacc.p; p.cacc = h->cacc.p; p.e = h->e.p; p.enc = h->enc.p; p.geo = h->geo.p;
            for (int i = 0; i < 6; ++i) p.wscale[i] = 1.0f;
            if (edge_uses_one_chain(NB, prec)) {     // the message kernel's own stream format (the primal pass of the divergence keeps the other one)
                p.stream = h->S(h->st_edge1[l]); p.nch = h->st_edge1[l].nch; p.vecs = h->edge_vecs1.p + (size_t)l * 21 * F;
                for (int i = 0; i < 6; ++i) p.wscale[i] = h->edge_scale[(size_t)l * 6 + i];
            }
            if (mrows) p.rows = mrows;
            Timed tm(h, TI_KERNEL_PAINN_EDGE);
#ifdef TI_STAMPS      // diagnostic build only: stamps of layer 2's launch, printed to stderr
            static DevBuf<unsigned long long> stamp_buf;
            const size_t n_st = 2048 + 2 * (size_t)groups + 16;
            if (l == 2 && std::getenv("TI_STAMPS_DUMP")) { if (stamp_buf.n < n_st) stamp_buf.alloc(n_st); HIP_CHECK(hipMemsetAsync(stamp_buf.p, 0, n_st * 8, st)); p.stamps = stamp_buf.p; }
            auto dump_stamps = [&]() {
                if (!p.stamps) return;
                std::vector<unsigned long long> hs(n_st);
                HIP_CHECK(hipStreamSynchronize(st));
                HIP_CHECK(hipMemcpy(hs.data(), stamp_buf.p, n_st * 8, hipMemcpyDeviceToHost));
                for (int w = 0; w < 32; ++w) {
                    if (!hs[(size_t)w * 64 + 1]) continue;
                    std::fprintf(stderr, "STAMP %d:", w);
                    for (int k = 1; k < 64 && hs[(size_t)w * 64 + k]; ++k) std::fprintf(stderr, " %llu", hs[(size_t)w * 64 + k] - hs[(size_t)w * 64 + k - 1]);
                    std::fprintf(stderr, "\n");
                }
                std::vector<double> clk;
                for (long long g2 = 0; g2 < groups; ++g2) { const auto c = hs[2048 + 2 * g2], r = hs[2048 + 2 * g2 + 1]; if (r) clk.push_back(100e6 * (double)c / (double)r); }
                std::sort(clk.begin(), clk.end());
                if (!clk.empty()) std::fprintf(stderr, "INKERNEL_CLOCK_GHZ median %.4f  p10 %.4f  p90 %.4f  waves %zu  layout %d  precision %d\n", clk[clk.size() / 2] / 1e9,
                                               clk[clk.size() / 10] / 1e9, clk[clk.size() * 9 / 10] / 1e9, clk.size(), h->active, prec);
            };
#endif
            if (h->active == 2) {
                p.part = h->part.p;
                HIP_CHECK(launch_pair(NB, l == 0, l == L - 1, prec, p, st, mrows != nullptr));
#ifdef TI_STAMPS
                dump_stamps();
#endif
                if (pair_uses_partials()) {
                PairReduceParams r{};
                r.part = h->part.p; r.plist = h->pair_plist.p; r.kmax = h->pair_kmax; r.G = h->G; r.A = A; r.F = F; r.nblk = h->nblk;
                r.has_c = l > 0 && !pair_folds_cross(prec); r.B = B; r.dsacc = h->dsacc.p; r.dvacc = h->dvacc.p; r.cacc = h->cacc.p;
                HIP_CHECK(launch_pair_reduce(r, st));
                }
            } else {
                HIP_CHECK(launch_edge(NB, l == 0, l == L - 1, prec, p, st, mrows != nullptr));
#ifdef TI_STAMPS
                dump_stamps();
#endif
            }
        }
        if (h->tap == 1 + 2 * l) return;
        if (jr) {
            {
                JvpNodeParams p{};
                p.stream = h->S(h->st_jvp_update[l]); p.nch = h->st_jvp_update[l].nch; p.vecs = h->upd_vecs.p + (size_t)l * 10 * F;
                p.N = N; p.s = h->s.p; p.v = h->v.p; p.dsacc = h->dsacc.p; p.dvacc = h->dvacc.p; p.cacc = h->cacc.p;
                p.ns = reinterpret_cast<float4*>(h->nodest.p);
                Timed tm(h, TI_KERNEL_PAINN_JVP_FILTER);
                HIP_CHECK(launch_jvp_node(NB, split, p, st));
            }
            JvpUpdateParams p{};
            p.stream = h->S(h->st_jvp_update[l]); p.nch = h->st_jvp_update[l].nch; p.vecs = h->upd_vecs.p + (size_t)l * 10 * F;
            p.N = VN; p.B = B; p.A = A; p.D = jr->D; p.G = h->G; p.has_next = l + 1 < L;
            p.v = h->v.p; p.cacc = h->cacc.p; p.ns = reinterpret_cast<const float4*>(h->nodest.p);
            p.ts = h->ts.p; p.tv = h->tv.p; p.tdsacc = h->tdsacc.p; p.tdvacc = h->tdvacc.p; p.tcacc = h->tcacc.p; p.tP = h->tP.p;
            p.zero_acc = !ft;
            Timed tm(h, TI_KERNEL_PAINN_JVP_UPDATE);
            HIP_CHECK(launch_jvp_update(NB, split, p, st));
        }
        {
            UpdateParams p{};
            p.stream = h->S(h->st_update[l]); p.nch = h->st_update[l].nch; p.vecs = h->upd_vecs.p + (size_t)l * 10 * F;
            p.N = N; p.s = h->s.p; p.v = h->v.p; p.dsacc = h->dsacc.p; p.dvacc = h->dvacc.p; p.cacc = h->cacc.p; p.P = h->P.p;
            p.first_layer = l == 0; p.zero_acc = !ft;
            // after a pair launch that folded the cross term into dvacc, the update kernel that reads neither cacc nor its cross product
            // (cacc is then not written in this layer; the tangent passes, which read it, run on directed launches only)
            const bool folded = h->nblk > 0 && h->active == 2 && l > 0 && pair_folds_cross(prec);
            Timed tm(h, TI_KERNEL_PAINN_UPDATE);
            HIP_CHECK(launch_update(NB, l + 1 < L, prec, p, st, folded));
        }
        if (h->tap == 2 + 2 * l) return;
    }
    if (jr) {
        JvpReadoutParams p{};
        p.stream = h->S(h->st_jvp_readout); p.nch = h->st_jvp_readout.nch; p.vecs = h->jvp_ro_vecs.p; p.b2_gate = h->b2_gate;
        p.N = VN; p.B = B; p.A = A; p.D = jr->D; p.G = h->G; p.s = h->s.p; p.v = h->v.p; p.ts = h->ts.p; p.tv = h->tv.p; p.tout = jr->tout;
        Timed tm(h, TI_KERNEL_PAINN_JVP_READOUT);
        HIP_CHECK(launch_jvp_readout(NB, split, p, st));
    }
    {
        ReadoutParams p{};
        p.stream = h->S(h->st_jvp_readout); p.nch = h->st_jvp_readout.nch; p.mlp = h->vec(h->readout);      // the 16-row image of W0, W1
        p.w2_gate = h->F(h->readout.W2 + F); p.b2_gate = h->b2_gate; p.Vr = h->F(h->Vr);
        p.N = N; p.s = h->s.p; p.v = h->v.p; p.out = out_dev;
        Timed tm(h, TI_KERNEL_PAINN_READOUT);
        HIP_CHECK(launch_readout(NB, prec, p, st));
    }
    if (nat) {            // a pad atom's drift (and the tangent of an explicit direction) is +0 whatever the network made of it
        HIP_CHECK(launch_zero_pads(out_dev, nat, B, 1, A, 3, st));
        if (jr && jr->D == 1) HIP_CHECK(launch_zero_pads(jr->tout, nat, B, 1, A, 3, st));
    }
}

// drift and exact divergence: 3A unit-seed tangent passes per molecule, in chunks that fit the tangent HBM budget
void painn_drift_div_dev(ti_handle* h, const float* x_dev, float t, const float* cond_dev, long long B, float* out_dev, float* div_dev,
                         const float* tv = nullptr)
{
    const int A = h->d.n_atoms, D = 3 * A;
    const long long chunk = jvp_chunk_molecules(h, D);
    for (long long b0 = 0; b0 < B; b0 += chunk) {
        const long long bc = std::min(chunk, B - b0);
        ensure_jvp_ws(h, bc, D);
        JvpRun jr{D, nullptr, h->tout.p};
        painn_drift_dev(h, x_dev + (size_t)b0 * A * 3, t, cond_dev ? cond_dev + (size_t)b0 * A * h->ncond : nullptr, bc,
                        out_dev + (size_t)b0 * A * 3, &jr, tv ? tv + b0 : nullptr, b0);
        if (h->ragged) HIP_CHECK(launch_div_reduce_ragged(h->tout.p, bc, D, h->G, h->natoms_dev.p + b0, div_dev + b0, h->stream));
        else HIP_CHECK(launch_div_reduce(h->tout.p, bc, D, h->G, div_dev + b0, h->stream));
    }
    h->last_B = std::min(chunk, B);
}

// Hutchinson probes of trajectories traj0 .. traj0 + B - 1 into h->probes [B][k][3A] (include/ti_hip.h ti_painn_drift_div_est),
// drawn once per API call: a rollout integrates with the same probes at every evaluation
void painn_make_probes(ti_handle* h, long long B, int k, uint64_t seed, long long traj0)
{
    const int n3 = 3 * h->d.n_atoms;
    if (h->probes.n < (size_t)B * k * n3) h->probes.alloc((size_t)B * k * n3);
    HIP_CHECK(launch_probes(h->probes.p, seed, traj0, B, k, n3, h->stream));
    if (h->ragged) HIP_CHECK(launch_zero_pads(h->probes.p, h->natoms_dev.p, B * k, k, h->d.n_atoms, 3, h->stream));      // pad components: 0
}

// drift and Hutchinson estimate of the divergence along the k probes of h->probes: D = k explicit tangent directions per molecule,
// in chunks sized for k directions
void painn_drift_div_est_dev(ti_handle* h, const float* x_dev, float t, const float* cond_dev, long long B, int k, float* out_dev,
                             float* est_dev, const float* tv = nullptr)
{
    const int A = h->d.n_atoms;
    const long long chunk = jvp_chunk_molecules(h, k);
    for (long long b0 = 0; b0 < B; b0 += chunk) {
        const long long bc = std::min(chunk, B - b0);
        ensure_jvp_ws(h, bc, k);
        const float* eps = h->probes.p + (size_t)b0 * k * A * 3;
        JvpRun jr{k, eps, h->tout.p};
        painn_drift_dev(h, x_dev + (size_t)b0 * A * 3, t, cond_dev ? cond_dev + (size_t)b0 * A * h->ncond : nullptr, bc,
                        out_dev + (size_t)b0 * A * 3, &jr, tv ? tv + b0 : nullptr, b0);
        HIP_CHECK(launch_hutch_reduce(h->tout.p, eps, bc, k, A, h->G, est_dev + b0, h->stream));
    }
    h->last_B = std::min(chunk, B);
}

// ------------------------------------------------------------------------------------------------ adw helpers
void adw_mlp_launch(ti_handle* h, bool embed, const float* a0, const float* in1, const float* emb, const int32_t* idx, float t,
                    long long rows, float* out, float* out_div)
{
    AdwParams p{};
    const Stream& s2 = embed ? h->st_be : h->st_net;
    p.stream = h->S(s2); p.nch = s2.nch;
    p.vecs = h->F(embed ? h->a_be_vecs : h->a_net_vecs);
    p.b_out = embed ? h->a_be_b_out : h->a_b_out; p.n_hidden = embed ? 1 : h->ad.num_layers - 1; p.B = rows;
    p.x = a0; p.in1 = in1; p.emb = emb; p.idx = idx; p.t = t; p.out = out; p.out_div = out_div;
    p.dim = embed ? 1 : h->a_dim;
    Timed tm(h, TI_KERNEL_ADW);
    HIP_CHECK(launch_adw(h->NB, h->ad.precision == TI_PREC_F16X2, p, h->stream));
}

// upload conditioning: dedupe (beta0, beta1) pairs on the host (the driver uses one pair, adw/sample.py:24)
long long adw_set_cond(ti_handle* h, const float* beta0, const float* beta1, long long B, int mem, std::vector<float>* u0_out = nullptr,
                       std::vector<float>* u1_out = nullptr)
{
    std::vector<float> b0(B), b1(B);
    if (mem == TI_MEM_DEVICE) {
        HIP_CHECK(hipMemcpy(b0.data(), beta0, B * sizeof(float), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(b1.data(), beta1, B * sizeof(float), hipMemcpyDeviceToHost));
    } else { std::memcpy(b0.data(), beta0, B * sizeof(float)); std::memcpy(b1.data(), beta1, B * sizeof(float)); }
    std::map<std::pair<float, float>, int> uniq;
    std::vector<int32_t> idx(B);
    std::vector<float> u0, u1;
    for (long long i = 0; i < B; ++i) {
        auto key = std::make_pair(b0[i], b1[i]);
        auto it = uniq.find(key);
        if (it == uniq.end()) { it = uniq.emplace(key, (int)u0.size()).first; u0.push_back(b0[i]); u1.push_back(b1[i]); }
        idx[i] = it->second;
    }
    h->aidx.upload(idx); h->abeta0_u.upload(u0); h->abeta1_u.upload(u1);
    h->aemb_u.alloc(u0.size());
    if (u0_out) *u0_out = u0;
    if (u1_out) *u1_out = u1;
    return (long long)u0.size();
}

// out_div (may be NULL): sum_i d b_i / d x_i, the divergence of the drift (beta_embed does not depend on x); x / out [B][d]
void adw_drift_dev(ti_handle* h, const float* x_dev, float t, long long U, long long B, float* out_dev, float* out_div)
{
    adw_mlp_launch(h, true, h->abeta0_u.p, h->abeta1_u.p, nullptr, nullptr, t, U, h->aemb_u.p, nullptr);   // beta_embed([b0, b1, t])
    adw_mlp_launch(h, false, x_dev, nullptr, h->aemb_u.p, h->aidx.p, t, B, out_dev, out_div);             // net([x, t, embed])
}

// per-row times: beta_embed([b0_i, b1_i, t_i]) per row (no dedupe: the time differs per row), then net([x_i, t_i, emb_i]).
// beta0 / beta1 / tv are device pointers [B].
void adw_drift_tv_dev(ti_handle* h, const float* x_dev, const float* tv, const float* beta0, const float* beta1, long long B, float* out_dev,
                      float* out_div)
{
    if (h->aemb_r.n < (size_t)B) h->aemb_r.alloc(B);
    adw_mlp_launch(h, true, beta0, beta1, tv, nullptr, 0.f, B, h->aemb_r.p, nullptr);          // a2 = emb[r] = t_r
    adw_mlp_launch(h, false, x_dev, tv, h->aemb_r.p, nullptr, 0.f, B, out_dev, out_div);       // a1 = in1[r] = t_r
}

// device copies of per-row beta0 / beta1 (host memory is staged into the handle; device pointers are used as they are)
void adw_rows_dev(ti_handle* h, const float* beta0, const float* beta1, long long B, int mem, const float** b0d, const float** b1d)
{
    if (mem == TI_MEM_DEVICE) { *b0d = beta0; *b1d = beta1; return; }
    if (h->abeta0_r.n < (size_t)B) { h->abeta0_r.alloc(B); h->abeta1_r.alloc(B); }
    HIP_CHECK(hipMemcpyAsync(h->abeta0_r.p, beta0, B * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(h->abeta1_r.p, beta1, B * sizeof(float), hipMemcpyHostToDevice, h->stream));
    *b0d = h->abeta0_r.p; *b1d = h->abeta1_r.p;
}

void ensure_adw_ws(ti_handle* h, long long B)
{
    if (B <= h->cap) return;
    const size_t n = (size_t)B * h->a_dim;             // state floats; the divergence / dlogp buffers hold one per particle
    h->ax.alloc(n); h->ab1.alloc(n); h->ab2.alloc(n); h->axt.alloc(n); h->adl.alloc(B); h->ad1.alloc(B); h->ad2.alloc(B);
    h->cap = B;
}

// ------------------------------------------------------------------------------------------------ shared rollout
// drift(x_dev, t, out_dev) evaluates the drift; state arrays have n floats; comps = floats per trajectory
// Optional second state of the reference ODE: d(dlogp)/dt = -div * 1e-2, returned * 1e2 (adw/thermo/integrators.py:38-68).
struct DlogpAux {
    float *dl = nullptr, *d1 = nullptr, *d2 = nullptr, *scaled = nullptr, *out = nullptr;
    size_t n_dl = 0;                              // entries of the second state (0: same as the first state's n)
    float div_scale = 1e-2f, out_scale = 100.0f;  // d(dlogp)/dt = -div_scale * div, written * out_scale
};

// Mixed-species batches (ti_painn_set_molecules): device atom counts [B] of a state [B][A][3], and the number of real floats in it.
// n == NULL: every entry is real.  The drift already returns +0 on pad atoms, so the fixed-step updates leave them where they are;
// what changes is the EM noise, the adaptive solvers' norms and their dense output.
struct Ragged { const int32_t* n = nullptr; int A = 0; size_t n_real = 0; };
Ragged ragged_of(const ti_handle* h) { return h->ragged ? Ragged{h->natoms_dev.p, h->d.n_atoms, (size_t)h->n_real * 3} : Ragged{}; }

// drift(x_dev, t, out_b, out_div) evaluates the drift (and the divergence if out_div != NULL); state arrays have n floats
// ------------------------------------------------------------------------------------------------ observables
int obs_floats_per_traj(const ti_handle* h) { return h->kind == 0 ? 3 * h->d.n_atoms : h->a_dim; }

// Validates desc [K][5] against the handle (before any device work) and uploads it with ref / select into set `which`.
int obs_upload(ti_handle* h, int which, const int32_t* desc, int K, const float* ref, const int32_t* select)
{
    if (K < 1) return fail(TI_E_ARG, "K must be >= 1");
    const int A = h->kind == 0 ? h->d.n_atoms : 1, dim = h->a_dim;
    bool rmsd = false;
    for (int k = 0; k < K; ++k) {
        const int32_t* d = desc + 5 * k;
        const int kind = d[0];
        if (kind < TI_OBS_RMSD || kind > TI_OBS_COORD) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": unknown kind " + std::to_string(kind));
        if (h->kind == 1) {
            if (kind != TI_OBS_COORD) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": an adw handle takes COORD(c) only");
            if (d[1] < 0 || d[1] >= dim) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": component outside 0.." + std::to_string(dim - 1));
            continue;
        }
        if (kind == TI_OBS_COORD) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": COORD(c) is for adw handles");
        if (kind == TI_OBS_RMSD) { rmsd = true; continue; }
        const int na = kind == TI_OBS_DIST ? 2 : kind == TI_OBS_ANGLE ? 3 : 4;
        for (int j = 0; j < na; ++j)
            if (d[1 + j] < 0 || d[1 + j] >= A) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": atom index outside 0.." + std::to_string(A - 1));
    }
    if (rmsd && !ref) return fail(TI_E_ARG, "an RMSD descriptor needs ref");
    set_device(h);
    ti_handle::ObsSet& o = h->obs[which];
    o.K = 0;
    o.desc.upload(std::vector<int32_t>(desc, desc + 5 * (size_t)K));
    o.has_ref = rmsd; o.has_sel = rmsd && select;
    if (o.has_ref) o.ref.upload(std::vector<float>(ref, ref + 3 * (size_t)A));
    if (o.has_sel) o.sel.upload(std::vector<int32_t>(select, select + A));
    o.K = K;
    return TI_OK;
}

// cv_dev [B][K] = the CVs of set `which` on x_dev [B][m]; enqueued on the handle's stream
void obs_cv_dev(ti_handle* h, int which, const float* x_dev, long long B, float* cv_dev)
{
    const ti_handle::ObsSet& o = h->obs[which];
    if (h->kind == 0 && h->emask_B > 0 && B != h->emask_B)
        throw std::invalid_argument("the molecule state in force is for " + std::to_string(h->emask_B) + " molecules, the call has " + std::to_string(B));
    ObsCvParams p{};
    p.x = x_dev; p.B = B; p.A = h->kind == 0 ? h->d.n_atoms : 1; p.m = obs_floats_per_traj(h); p.K = o.K;
    p.desc = o.desc.p; p.ref = o.has_ref ? o.ref.p : nullptr; p.sel = o.has_sel ? o.sel.p : nullptr;
    p.n_atoms = h->kind == 0 && h->ragged ? h->natoms_dev.p : nullptr;
    p.cv = cv_dev;
    HIP_CHECK(launch_obs_cv(p, h->stream));
}

// The attached observer of a rollout over B trajectories: at(i, x) writes the CV row of grid point i when the observer wants one.
struct Observer {
    ti_handle* h; long long B; int N; int64_t row = 0;
    bool on() const { return h->obs[1].K > 0; }
    bool wants(int i) const { return on() && (h->obs_every > 0 ? (i % h->obs_every == 0 || i == N - 1) : i == N - 1); }
    void at(int i, const float* x_dev)
    {
        if (!wants(i)) return;
        const size_t nk = (size_t)B * h->obs[1].K;
        float* dst = h->obs_out + (size_t)(row++) * nk;
        if (h->obs_mem == TI_MEM_DEVICE) { obs_cv_dev(h, 1, x_dev, B, dst); return; }
        if (h->obs_cv.n < nk) h->obs_cv.alloc(nk);
        obs_cv_dev(h, 1, x_dev, B, h->obs_cv.p);
        HIP_CHECK(hipMemcpyAsync(dst, h->obs_cv.p, nk * sizeof(float), hipMemcpyDeviceToHost, h->stream));     // pageable: done on return
    }
};

template <typename Drift>
int rollout_common(ti_handle* h, const ti_rollout_desc* rd, float* x, float* b1, float* b2, float* xt, size_t n, long long B, int comps,
                   int atoms_for_com, float* out_path, int64_t* n_fevals, Drift&& drift, DlogpAux aux = DlogpAux(), Ragged rg = Ragged())
{
    hipStream_t st = h->stream;
    const hipMemcpyKind out_kind = rd->mem == TI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    int64_t row = 0, fe = 0;
    const size_t ndl = aux.n_dl ? aux.n_dl : n;
    if (aux.dl) HIP_CHECK(hipMemsetAsync(aux.dl, 0, ndl * sizeof(float), st));
    auto save = [&]() {
        if (aux.dl) {
            HIP_CHECK(launch_scale(aux.scaled, aux.dl, aux.out_scale, (long long)ndl, st));
            HIP_CHECK(hipMemcpyAsync(aux.out + (size_t)row * ndl, aux.scaled, ndl * sizeof(float), out_kind, st));
        }
        HIP_CHECK(hipMemcpyAsync(out_path + (size_t)(row++) * n, x, n * sizeof(float), out_kind, st));
    };
    Observer obs{h, B, rd->n_step};
    if (rd->save_every > 0) save();
    if (obs.on()) obs.at(0, x);
    for (int k = 0; k < rd->n_step - 1; ++k) {
        const float dt = rd->t_grid[k + 1] - rd->t_grid[k];
        drift(x, rd->t_grid[k], b1, aux.d1); ++fe;
        if (rd->scheme == TI_SCHEME_HEUN) {
            { Timed tm(h, TI_KERNEL_INTEGRATE); HIP_CHECK(launch_axpy(xt, x, dt, b1, (long long)n, st)); }
            drift(xt, rd->t_grid[k + 1], b2, aux.d2); ++fe;
            { Timed tm(h, TI_KERNEL_INTEGRATE); HIP_CHECK(launch_heun(x, 0.5f * dt, b1, b2, (long long)n, st)); }
            if (aux.dl) HIP_CHECK(launch_heun(aux.dl, -0.5f * dt * aux.div_scale, aux.d1, aux.d2, (long long)ndl, st));
        } else {
            Timed tm(h, TI_KERNEL_INTEGRATE);
            HIP_CHECK(launch_axpy(x, x, dt, b1, (long long)n, st));
            if (aux.dl) HIP_CHECK(launch_axpy(aux.dl, aux.dl, -dt * aux.div_scale, aux.d1, (long long)ndl, st));
            if (rd->scheme == TI_SCHEME_EM && rd->eps > 0.0f && rg.n)
                HIP_CHECK(launch_noise_ragged(x, std::sqrt(2.0f * rd->eps * std::fabs(dt)), rd->seed, rd->traj_offset, (int)(rd->step_offset + k), B, rg.A,
                                              rd->com_free_noise ? 1 : 0, rg.n, st));
            else if (rd->scheme == TI_SCHEME_EM && rd->eps > 0.0f)
                HIP_CHECK(launch_noise(x, std::sqrt(2.0f * rd->eps * std::fabs(dt)), rd->seed, rd->traj_offset, (int)(rd->step_offset + k), B, comps,
                                       rd->com_free_noise ? atoms_for_com : 0, st));
        }
        const int step = k + 1;
        if (rd->save_every > 0 && (step % rd->save_every == 0 || step == rd->n_step - 1)) save();
        if (obs.on()) obs.at(step, x);
    }
    if (rd->save_every <= 0) save();
    HIP_CHECK(hipMemsetAsync(h->nanflag.p, 0, sizeof(int), st));
    HIP_CHECK(launch_nan_check(x, (long long)n, h->nanflag.p, st));
    int flag = 0;
    HIP_CHECK(hipMemcpyAsync(&flag, h->nanflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (n_fevals) *n_fevals = fe;
    return flag ? fail(TI_E_NAN, "non-finite value in the final state") : TI_OK;
}

// ---- Runge-Kutta drivers on top of the same drift callback: torchdiffeq 0.2.5's `dopri5` (adaptive), `midpoint`, `rk4`
// (include/ti_hip.h TI_SCHEME_*).  State = segment 0 (x, n floats) and optionally segment 1 (dlogp, aux.n_dl floats) with
// right-hand side (b, -div_scale * div); a decreasing grid is integrated in s = -t with f'(s, y) = -f(-s, y) like
// torchdiffeq's _ReverseFunc.  Times and step sizes are fp64 on the host and enter state arithmetic as fp32, as there.
namespace dp5 {
constexpr double alpha[6] = {1. / 5, 3. / 10, 4. / 5, 8. / 9, 1., 1.};
constexpr double beta[6][6] = {{1. / 5},
                               {3. / 40, 9. / 40},
                               {44. / 45, -56. / 15, 32. / 9},
                               {19372. / 6561, -25360. / 2187, 64448. / 6561, -212. / 729},
                               {9017. / 3168, -355. / 33, 46732. / 5247, 49. / 176, -5103. / 18656},
                               {35. / 384, 0., 500. / 1113, 125. / 192, -2187. / 6784, 11. / 84}};
constexpr double c_error[7] = {35. / 384 - 1951. / 21600, 0., 500. / 1113 - 22642. / 50085, 125. / 192 - 451. / 720,
                               -2187. / 6784 - -12231. / 42400, 11. / 84 - 649. / 6300, -1. / 60};
constexpr double c_mid[7] = {6025192743. / 30085553152. / 2, 0., 51252292925. / 65400821598. / 2, -2691868925. / 45128329728. / 2,
                             187940372067. / 1594534317056. / 2, -1776094331. / 19743644256. / 2, 11237099. / 235043384. / 2};
}  // namespace dp5

template <typename Drift>
int rollout_rk(ti_handle* h, const ti_rollout_desc* rd, float* x, size_t n, float* out_path, int64_t* n_fevals, Drift&& drift,
               DlogpAux aux = DlogpAux(), Ragged rg = Ragged())
{
    hipStream_t st = h->stream;
    const hipMemcpyKind out_kind = rd->mem == TI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const int nseg = aux.dl ? 2 : 1;
    const size_t ndl = aux.dl ? (aux.n_dl ? aux.n_dl : n) : 0;
    const size_t sn[2] = {n, ndl};
    // workspace: per segment k[7], ytmp, ynew, coef[5]
    const size_t per = 14;
    if (h->rk_ws.n < per * (n + ndl)) h->rk_ws.alloc(per * (n + ndl));
    if (h->rk_red.n < (size_t)RED_PARTIALS + 8) h->rk_red.alloc(RED_PARTIALS + 8);
    float* y[2] = {x, aux.dl};
    float *k[2][7] = {}, *ytmp[2] = {}, *ynew[2] = {}, *coef[2] = {};
    struct Pair { float* p[2]; operator float* const*() const { return p; } };
    auto KP = [&](int j) { return Pair{{k[0][j], k[1][j]}}; };
    {
        float* w = h->rk_ws.p;
        for (int s2 = 0; s2 < nseg; ++s2) {
            for (int j = 0; j < 7; ++j) { k[s2][j] = w; w += sn[s2]; }
            ytmp[s2] = w; w += sn[s2]; ynew[s2] = w; w += sn[s2]; coef[s2] = w; w += 5 * sn[s2];
        }
    }
    if (aux.dl) HIP_CHECK(hipMemsetAsync(aux.dl, 0, ndl * sizeof(float), st));
    const int N = rd->n_step;
    const double sign = (N > 1 && rd->t_grid[1] < rd->t_grid[0]) ? -1.0 : 1.0;
    int64_t fe = 0, row = 0;
    // f(s, y) for every segment; `ti` is the fp32 stage time in the (possibly negated) integration variable
    auto F = [&](float ti, float* const* yin, float* const* kout) {
        drift(yin[0], (float)(sign * (double)ti), kout[0], aux.dl ? aux.d1 : nullptr); ++fe;
        if (aux.dl) HIP_CHECK(launch_scale(kout[1], aux.d1, (float)(-sign) * aux.div_scale, (long long)ndl, st));
        if (sign < 0) HIP_CHECK(launch_scale(kout[0], kout[0], -1.0f, (long long)n, st));
    };
    auto save_from = [&](float* const* src) {
        if (aux.dl) {
            HIP_CHECK(launch_scale(aux.scaled, src[1], aux.out_scale, (long long)ndl, st));
            HIP_CHECK(hipMemcpyAsync(aux.out + (size_t)row * ndl, aux.scaled, ndl * sizeof(float), out_kind, st));
        }
        HIP_CHECK(hipMemcpyAsync(out_path + (size_t)(row++) * n, src[0], n * sizeof(float), out_kind, st));
    };
    auto wants_row = [&](int i) { return rd->save_every > 0 ? (i % rd->save_every == 0 || i == N - 1) : i == N - 1; };
    auto comb = [&](int s2, int nk, const double* c, double scale) {
        RkComb r{};
        r.nk = nk;
        for (int j = 0; j < nk; ++j) { r.k[j] = k[s2][j]; r.c[j] = (float)c[j] * (float)scale; }       // beta_ij * dt in fp32
        return r;
    };
    double* red = h->rk_red.p;
    auto fetch = [&]() { double v = 0; HIP_CHECK(hipMemcpyAsync(&v, red + RED_PARTIALS, sizeof(double), hipMemcpyDeviceToHost, st)); HIP_CHECK(hipStreamSynchronize(st)); return v; };
    const float rtol = rd->rtol, atol = rd->atol;
    Observer obs{h, (long long)(n / (size_t)obs_floats_per_traj(h)), N};
    if (wants_row(0)) save_from(y);
    if (obs.on()) obs.at(0, y[0]);

    if (rd->scheme == TI_SCHEME_MIDPOINT || rd->scheme == TI_SCHEME_RK4) {
        // FixedGridODESolver with step_size = None: one step per grid interval (solvers.py; fixed_grid.py Midpoint / RK4)
        for (int i = 0; i + 1 < N; ++i) {
            const float t0 = (float)(sign * rd->t_grid[i]), t1 = (float)(sign * rd->t_grid[i + 1]), dt = t1 - t0;
            F(t0, y, KP(0));
            if (rd->scheme == TI_SCHEME_MIDPOINT) {
                const double half[1] = {0.5};
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 1, half, dt), (long long)sn[s2], st));
                F(t0 + 0.5f * dt, ytmp, KP(1));
                const double one[2] = {0., 1.};
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(y[s2], y[s2], comb(s2, 2, one, dt), (long long)sn[s2], st));
            } else {                        // rk4_alt_step_func: the 3/8 rule
                const double c2[1] = {1. / 3}, c3[2] = {-1. / 3, 1.}, c4[3] = {1., -1., 1.}, cs[4] = {0.125, 0.375, 0.375, 0.125};
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 1, c2, dt), (long long)sn[s2], st));
                F(t0 + dt * (1.0f / 3.0f), ytmp, KP(1));
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 2, c3, dt), (long long)sn[s2], st));
                F(t0 + dt * (2.0f / 3.0f), ytmp, KP(2));
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 3, c4, dt), (long long)sn[s2], st));
                F(t1, ytmp, KP(3));
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(y[s2], y[s2], comb(s2, 4, cs, dt), (long long)sn[s2], st));
            }
            if (wants_row(i + 1)) save_from(y);
            if (obs.on()) obs.at(i + 1, y[0]);
        }
    } else {
        // ---- dopri5: RKAdaptiveStepsizeODESolver (rk_common.py) ----
        auto norm_of = [&](auto&& launch_one) {        // mixed norm: max over segments of the rms (misc.py _mixed_norm / _rms_norm)
            double best = 0.0;
            for (int s2 = 0; s2 < nseg; ++s2) {
                launch_one(s2);
                best = std::max(best, std::sqrt(fetch() / (double)(s2 == 0 && rg.n ? rg.n_real : sn[s2])));      // rms over the real entries
            }
            return best;
        };
        const double t_first = sign * (double)rd->t_grid[0];
        F((float)t_first, y, KP(0));
        // _select_initial_step(func, t0, y0, order - 1 = 4, rtol, atol, norm, f0)
        // segment 0 of a mixed-species batch takes the ragged sums (pad entries skipped)
        auto scaled_sumsq = [&](int s2, const float* a, const float* b2) {
            if (s2 == 0 && rg.n) HIP_CHECK(launch_scaled_sumsq_ragged(red + RED_PARTIALS, red, a, b2, y[s2], rtol, atol, (long long)sn[s2], rg.n, 3 * rg.A, st));
            else HIP_CHECK(launch_scaled_sumsq(red + RED_PARTIALS, red, a, b2, y[s2], rtol, atol, (long long)sn[s2], st));
        };
        const double d0 = norm_of([&](int s2) { scaled_sumsq(s2, y[s2], nullptr); });
        const double d1 = norm_of([&](int s2) { scaled_sumsq(s2, k[s2][0], nullptr); });
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        {
            const double one[1] = {1.};
            for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 1, one, h0), (long long)sn[s2], st));
        }
        F((float)(t_first + h0), ytmp, KP(1));
        const double d2 = norm_of([&](int s2) { scaled_sumsq(s2, k[s2][1], k[s2][0]); }) / h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3) : std::pow(0.01 / std::max(d1, d2), 1.0 / 5.0);
        double dt = std::min(100.0 * h0, h1);
        double t0 = t_first, t1 = t_first;            // interpolation interval of the last accepted step
        long long attempts = 0;
        for (int i = 1; i < N; ++i) {
            const double next_t = sign * (double)rd->t_grid[i];
            while (next_t > t1) {
                if (++attempts > 10000000LL) return fail(TI_E_NAN, "dopri5: more than 1e7 step attempts");
                const double ts = t1, te = ts + dt;
                if (!(te > ts)) return fail(TI_E_NAN, "dopri5: step size underflow (dt = " + std::to_string(dt) + ")");
                const float tsf = (float)ts, dtf = (float)dt, tef = (float)te;
                for (int sidx = 0; sidx < 6; ++sidx) {                       // _runge_kutta_step
                    const float ti = dp5::alpha[sidx] == 1.0 ? std::nextafterf(tef, tef - 1.0f) : tsf + (float)dp5::alpha[sidx] * dtf;
                    float* const* dst = sidx == 5 ? ynew : ytmp;             // c_sol == beta[5]: the last stage input IS y1
                    for (int s2 = 0; s2 < nseg; ++s2)
                        HIP_CHECK(launch_rk_combo(dst[s2], y[s2], comb(s2, sidx + 1, dp5::beta[sidx], dtf), (long long)sn[s2], st));
                    F(ti, dst, KP(sidx + 1));
                }
                const double ratio = norm_of([&](int s2) {                  // _compute_error_ratio
                    if (s2 == 0 && rg.n) HIP_CHECK(launch_rk_ratio_sumsq_ragged(red + RED_PARTIALS, red, y[s2], ynew[s2], comb(s2, 7, dp5::c_error, dtf), rtol, atol, (long long)sn[s2], rg.n, 3 * rg.A, st));
                    else HIP_CHECK(launch_rk_ratio_sumsq(red + RED_PARTIALS, red, y[s2], ynew[s2], comb(s2, 7, dp5::c_error, dtf), rtol, atol, (long long)sn[s2], st));
                });
                if (!(ratio == ratio)) return fail(TI_E_NAN, "dopri5: non-finite error estimate");
                if (ratio <= 1.0) {                                          // accept: dense output, FSAL
                    for (int s2 = 0; s2 < nseg; ++s2) {
                        HIP_CHECK(launch_interp_fit(coef[s2], y[s2], ynew[s2], k[s2][0], k[s2][6], comb(s2, 7, dp5::c_mid, dtf), dtf, (long long)sn[s2], st));
                        HIP_CHECK(hipMemcpyAsync(y[s2], ynew[s2], sn[s2] * sizeof(float), hipMemcpyDeviceToDevice, st));
                        std::swap(k[s2][0], k[s2][6]);
                    }
                    t0 = ts; t1 = te;
                }
                // _optimal_step_size(dt, ratio, safety 0.9, ifactor 10, dfactor 0.2, order 5)
                if (ratio == 0.0) dt *= 10.0;
                else dt *= std::min(10.0, std::max(0.9 / std::pow(ratio, 0.2), ratio < 1.0 ? 1.0 : 0.2));
            }
            if (wants_row(i)) {                                              // _interp_evaluate at the requested time
                const float xrel = (float)((next_t - t0) / (t1 - t0));
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_interp_eval(ytmp[s2], coef[s2], xrel, (long long)sn[s2], st));
                if (rg.n) HIP_CHECK(launch_copy_pads(ytmp[0], y[0], rg.n, (long long)(n / (3 * rg.A)), rg.A, 3, st));      // pads: the state, not its fit
                save_from(ytmp);
                if (obs.on()) obs.at(i, ytmp[0]);
            } else if (obs.wants(i)) {                                       // an observer row where no path row is written: x only
                const float xrel = (float)((next_t - t0) / (t1 - t0));
                HIP_CHECK(launch_interp_eval(ytmp[0], coef[0], xrel, (long long)sn[0], st));
                obs.at(i, ytmp[0]);
            }
        }
    }
    HIP_CHECK(hipMemsetAsync(h->nanflag.p, 0, sizeof(int), st));
    HIP_CHECK(launch_nan_check(x, (long long)n, h->nanflag.p, st));
    int flag = 0;
    HIP_CHECK(hipMemcpyAsync(&flag, h->nanflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (n_fevals) *n_fevals = fe;
    return flag ? fail(TI_E_NAN, "non-finite value in the final state") : TI_OK;
}

// ---- dopri5 with per-trajectory step control (TI_SCHEME_DOPRI5_TRAJ): trajectory b of m floats (plus its dlogp entry) runs the
// algorithm of rollout_rk above on its own -- initial step from its own norms, its own accept / reject decisions, step sizes and
// dense output (ode_kernels.hip, TrajRkParams) -- inside batched drift launches that take one stage time per trajectory
// (drift(x, tv, out, out_div), tv a device array [B]).  The batch takes as many attempts as its hardest trajectory; a finished
// (frozen) trajectory is evaluated along but never written again.  One small status read-back per attempt, as in rollout_rk.
template <typename DriftTv>
int rollout_rk_traj(ti_handle* h, const ti_rollout_desc* rd, float* x, long long B, long long m, float* out_path, int64_t* n_fevals,
                    DriftTv&& drift, DlogpAux aux = DlogpAux(), Ragged rg = Ragged())
{
    hipStream_t st = h->stream;
    const int nseg = aux.dl ? 2 : 1, N = rd->n_step;
    const size_t n = (size_t)B * m, ndl = aux.dl ? (size_t)B : 0, sn[2] = {n, ndl};
    const size_t per = 14;                                   // per segment k[7], ytmp, ynew, coef[5]
    if (h->rk_ws.n < per * (n + ndl)) h->rk_ws.alloc(per * (n + ndl));
    if (h->rk_ctl.n < (size_t)B) h->rk_ctl.alloc(B);
    if (h->rk_tv.n < (size_t)B) h->rk_tv.alloc(B);
    if (h->rk_status.n < (size_t)TRAJ_ST_N) h->rk_status.alloc(TRAJ_ST_N);
    const int total_rows = (int)ti_rollout_rows(N, rd->save_every);
    const bool host_out = rd->mem == TI_MEM_HOST;            // rows are written on the device and copied out as they complete
    float* path_dev = out_path;
    float* dl_dev = aux.out;
    if (host_out) {
        if (h->rk_path.n < (size_t)total_rows * n) h->rk_path.alloc((size_t)total_rows * n);
        path_dev = h->rk_path.p;
        if (aux.dl) { if (h->rk_dpath.n < (size_t)total_rows * ndl) h->rk_dpath.alloc((size_t)total_rows * ndl); dl_dev = h->rk_dpath.p; }
    }
    const double sign = (N > 1 && rd->t_grid[1] < rd->t_grid[0]) ? -1.0 : 1.0;
    {
        std::vector<double> g(N);
        for (int i = 0; i < N; ++i) g[i] = sign * (double)rd->t_grid[i];
        h->rk_grid.upload(g);
    }
    TrajRkParams p{};
    p.nseg = nseg; p.B = B; p.ctl = h->rk_ctl.p; p.tv = h->rk_tv.p; p.status = h->rk_status.p; p.grid = h->rk_grid.p;
    p.n_grid = N; p.save_every = rd->save_every; p.total_rows = total_rows; p.sign = sign; p.t_first = sign * (double)rd->t_grid[0];
    p.rtol = rd->rtol; p.atol = rd->atol; p.max_attempts = 10000000LL;
    {
        float* w = h->rk_ws.p;
        float* y[2] = {x, aux.dl};
        for (int s2 = 0; s2 < nseg; ++s2) {
            TrajSeg& g = p.seg[s2];
            for (int j = 0; j < 7; ++j) { g.k[j] = w; w += sn[s2]; }
            g.ytmp = w; w += sn[s2]; g.ynew = w; w += sn[s2]; g.coef = w; w += 5 * sn[s2];
            g.y = y[s2]; g.m = s2 ? 1 : m; g.out = s2 ? dl_dev : path_dev; g.out_scale = s2 ? aux.out_scale : 1.0f;
        }
    }
    if (aux.dl) HIP_CHECK(hipMemsetAsync(aux.dl, 0, ndl * sizeof(float), st));
    int64_t fe = 0;
    auto F = [&](int which) {                                // k[which] = f(s, y_in) at the stage times in rk_tv
        float* yin[2] = {which == 0 ? p.seg[0].y : which == 6 ? p.seg[0].ynew : p.seg[0].ytmp,
                         aux.dl ? (which == 0 ? p.seg[1].y : which == 6 ? p.seg[1].ynew : p.seg[1].ytmp) : nullptr};
        drift(yin[0], h->rk_tv.p, p.seg[0].k[which], aux.dl ? aux.d1 : nullptr); ++fe;
        if (aux.dl) HIP_CHECK(launch_scale(p.seg[1].k[which], aux.d1, (float)(-sign) * aux.div_scale, (long long)ndl, st));
        if (sign < 0) HIP_CHECK(launch_scale(p.seg[0].k[which], p.seg[0].k[which], -1.0f, (long long)n, st));
    };
    auto wants_row0 = rd->save_every > 0 || N == 1;
    if (wants_row0) {
        HIP_CHECK(hipMemcpyAsync(path_dev, x, n * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (aux.dl) HIP_CHECK(launch_scale(dl_dev, aux.dl, aux.out_scale, (long long)ndl, st));
    }
    {
        const float t0f = (float)(sign * (double)(float)p.t_first);
        uint32_t bits; std::memcpy(&bits, &t0f, 4);
        HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->rk_tv.p), (int)bits, (size_t)B, st));
    }
    F(0);
    HIP_CHECK(rg.n ? launch_traj_init_ragged(p, 0, rg.n, st) : launch_traj_init(p, 0, st));                    // _select_initial_step, per trajectory
    F(1);
    HIP_CHECK(rg.n ? launch_traj_init_ragged(p, 1, rg.n, st) : launch_traj_init(p, 1, st));
    float c_err[7], c_mid[7];
    for (int j = 0; j < 7; ++j) { c_err[j] = (float)dp5::c_error[j]; c_mid[j] = (float)dp5::c_mid[j]; }
    int status[TRAJ_ST_N] = {0, 0, INT_MAX, INT_MAX, INT_MAX, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(h->rk_status.p, status, sizeof(status), hipMemcpyHostToDevice, st));
    int copied = 0;                                           // rows already copied to the host
    auto copy_rows = [&](int upto) {
        if (!host_out || upto <= copied) return;
        HIP_CHECK(hipMemcpyAsync(out_path + (size_t)copied * n, path_dev + (size_t)copied * n, (size_t)(upto - copied) * n * sizeof(float),
                                 hipMemcpyDeviceToHost, st));
        if (aux.dl) HIP_CHECK(hipMemcpyAsync(aux.out + (size_t)copied * ndl, dl_dev + (size_t)copied * ndl, (size_t)(upto - copied) * ndl * sizeof(float),
                                             hipMemcpyDeviceToHost, st));
        copied = upto;
    };
    for (bool active = N > 1; active;) {
        HIP_CHECK(hipMemsetAsync(h->rk_status.p, 0, 2 * sizeof(int), st));        // active count, rows missing
        for (int sidx = 0; sidx < 6; ++sidx) {                                   // _runge_kutta_step, every trajectory with its own dt
            float c[6];
            for (int j = 0; j <= sidx; ++j) c[j] = (float)dp5::beta[sidx][j];
            HIP_CHECK(rg.n ? launch_traj_stage_ragged(p, c, sidx + 1, (float)dp5::alpha[sidx], dp5::alpha[sidx] == 1.0, sidx == 5, sidx == 0, rg.n, st)
                           : launch_traj_stage(p, c, sidx + 1, (float)dp5::alpha[sidx], dp5::alpha[sidx] == 1.0, sidx == 5, sidx == 0, st));
            F(sidx == 5 ? 6 : sidx + 1);
        }
        HIP_CHECK(rg.n ? launch_traj_advance_ragged(p, c_err, c_mid, rg.n, st) : launch_traj_advance(p, c_err, c_mid, st));
        HIP_CHECK(hipMemcpyAsync(status, h->rk_status.p, sizeof(status), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (status[TRAJ_ST_UNDERFLOW] != INT_MAX)
            return fail(TI_E_NAN, "dopri5 (per trajectory): step size underflow in trajectory " + std::to_string(status[TRAJ_ST_UNDERFLOW]));
        if (status[TRAJ_ST_NAN] != INT_MAX)
            return fail(TI_E_NAN, "dopri5 (per trajectory): non-finite error estimate in trajectory " + std::to_string(status[TRAJ_ST_NAN]));
        if (status[TRAJ_ST_LIMIT] != INT_MAX)
            return fail(TI_E_NAN, "dopri5 (per trajectory): more than 1e7 step attempts in trajectory " + std::to_string(status[TRAJ_ST_LIMIT]));
        copy_rows(total_rows - status[TRAJ_ST_MISSING]);                          // completed-row watermark
        active = status[TRAJ_ST_ACTIVE] > 0;
    }
    copy_rows(total_rows);
    std::vector<TrajCtl> ctl(B);
    HIP_CHECK(hipMemcpyAsync(ctl.data(), h->rk_ctl.p, (size_t)B * sizeof(TrajCtl), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemsetAsync(h->nanflag.p, 0, sizeof(int), st));
    HIP_CHECK(launch_nan_check(x, (long long)n, h->nanflag.p, st));
    int flag = 0;
    HIP_CHECK(hipMemcpyAsync(&flag, h->nanflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    h->traj_accepted.resize(B); h->traj_rejected.resize(B);
    for (long long b = 0; b < B; ++b) { h->traj_accepted[b] = ctl[b].accepted; h->traj_rejected[b] = ctl[b].rejected; }
    if (n_fevals) *n_fevals = fe;
    return flag ? fail(TI_E_NAN, "non-finite value in the final state") : TI_OK;
}

int check_rollout_desc(const ti_rollout_desc* rd)
{
    if (!rd || !rd->t_grid) return fail(TI_E_ARG, "rollout desc / t_grid is NULL");
    if (rd->n_step < 1) return fail(TI_E_ARG, "n_step must be >= 1");
    if (rd->scheme < TI_SCHEME_EULER || rd->scheme > TI_SCHEME_DOPRI5_TRAJ) return fail(TI_E_ARG, "unknown scheme");
    const bool adaptive = rd->scheme == TI_SCHEME_DOPRI5 || rd->scheme == TI_SCHEME_DOPRI5_TRAJ;
    if (adaptive && !(rd->rtol > 0.f && rd->atol > 0.f)) return fail(TI_E_ARG, "dopri5 needs rtol > 0 and atol > 0");
    if (rd->scheme >= TI_SCHEME_DOPRI5)
        for (int k = 0; k + 2 < rd->n_step; ++k)
            if ((rd->t_grid[k + 1] > rd->t_grid[k]) != (rd->t_grid[k + 2] > rd->t_grid[k + 1]) || rd->t_grid[k + 1] == rd->t_grid[k])
                return fail(TI_E_ARG, "t_grid must be strictly monotonic");
    if (rd->mem != TI_MEM_HOST && rd->mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem kind");
    if (rd->eps < 0.f) return fail(TI_E_ARG, "eps must be >= 0");
    if (rd->step_offset < 0 || rd->step_offset + rd->n_step > 0x7fffffffLL) return fail(TI_E_ARG, "step_offset out of range");
    return TI_OK;
}

template <typename Fn>
int guarded(Fn&& fn)
{
    try { return fn(); }
    catch (const HipError& e) { return fail(TI_E_HIP, e.what()); }
    catch (const Unsupported& e) { return fail(TI_E_UNSUPPORTED, e.what()); }
    catch (const std::bad_alloc&) { return fail(TI_E_ALLOC, "host allocation failed"); }
    catch (const std::exception& e) { return fail(TI_E_ARG, e.what()); }
}

ti_handle* new_handle(int kind, int device)
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

}  // namespace

// ====================================================================================================== C ABI
extern "C" {

int ti_version(void) { return TI_ABI_VERSION; }

int ti_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

const char* ti_last_error(void) { return g_err.c_str(); }

int64_t ti_rollout_rows(int32_t n_step, int32_t save_every)
{
    if (save_every <= 0) return 1;
    const int64_t steps = n_step - 1;
    return steps / save_every + 1 + (steps % save_every != 0);
}

ti_handle* ti_painn_create(const ti_painn_desc* d, const float* weights, size_t n_weights, const int32_t* edge_src,
                           const int32_t* edge_dst, const int32_t* edge_type, const int32_t* atom_ids, int device)
{
    ti_handle* out = nullptr;
    const int rc = guarded([&]() -> int {
        if (!d || !weights || !atom_ids) return fail(TI_E_ARG, "NULL argument");
        const int F = d->n_features, L = d->n_layers, A = d->n_atoms, E = d->n_edges;
        if (F != 32 && F != 64 && F != 128 && F != 256) return fail(TI_E_UNSUPPORTED, "n_features must be 32, 64, 128 or 256");
        if (L < 1) return fail(TI_E_ARG, "n_layers must be >= 1");
        if (A < 1 || A > 32) return fail(TI_E_UNSUPPORTED, "n_atoms must be in 1..32 (the reference caps it at n_types = 25)");
        if (E < 0 || (E > 0 && (!edge_src || !edge_dst || !edge_type))) return fail(TI_E_ARG, "edge arrays missing");
        if (d->variant < 0 || d->variant > 2) return fail(TI_E_ARG, "unknown variant");
        if (d->n_types < 1) return fail(TI_E_ARG, "n_types must be >= 1");
        if (d->precision != TI_PREC_F32 && d->precision != TI_PREC_F16X2 && d->precision != TI_PREC_F16) return fail(TI_E_ARG, "unknown precision");
        for (int k = 0; k < E; ++k)
            if (edge_src[k] < 0 || edge_src[k] >= A || edge_dst[k] < 0 || edge_dst[k] >= A || edge_type[k] < 0 || edge_type[k] > 3)
                return fail(TI_E_ARG, "edge index / type out of range");
        for (int a = 0; a < A; ++a) if (atom_ids[a] < 0 || atom_ids[a] >= d->n_types) return fail(TI_E_ARG, "atom id out of range");
        std::unique_ptr<ti_handle> h(new_handle(0, device));
        h->d = *d; h->NB = F / 32;
        h->nE = d->variant == TI_VARIANT_AMBIENT ? 4 : d->variant == TI_VARIANT_LATENT_MULTI ? 3 : 2;
        h->ncond = d->variant == TI_VARIANT_AMBIENT ? 2 : d->variant == TI_VARIANT_LATENT_MULTI ? 1 : 0;
        // canonical layout offsets (include/ti_hip.h)
        size_t o = 0;
        h->edge_emb = o; o += 4 * (size_t)F; h->atom_emb = o; o += (size_t)d->n_types * F;
        o = take_mlp(h->embed, o, h->nE * F, F, F);
        h->phi.resize(L); h->w.resize(L); h->upd.resize(L); h->U.resize(L); h->V.resize(L);
        for (int l = 0; l < L; ++l) {
            o = take_mlp(h->phi[l], o, 2 * F, F, 5 * F); o = take_mlp(h->w[l], o, F, F, 5 * F);
            h->U[l] = o; o += (size_t)F * F; h->V[l] = o; o += (size_t)F * F;
            o = take_mlp(h->upd[l], o, 2 * F, F, 3 * F);
        }
        o = take_mlp(h->readout, o, F, F, 2);
        h->Vr = o; o += F;
        if (o != n_weights) return fail(TI_E_ARG, "weight count mismatch: expected " + std::to_string(o) + ", got " + std::to_string(n_weights));
        h->b2_gate = weights[h->readout.b2 + 1];
        // natural-order copy; Vr follows the 2-float readout bias in the canonical layout, so a 16-byte aligned copy of it
        // is appended for the kernels' float4 loads
        std::vector<float> flat(weights, weights + n_weights);
        if (d->precision != TI_PREC_F32)            // the weights' hi halves are plain fp16: refuse what would round to inf
            for (size_t i = 0; i < n_weights; ++i)
                if (!(std::fabs(weights[i]) < 65504.0f))
                    return fail(TI_E_UNSUPPORTED, "precisions f16x2 / f16 need every weight to be finite and below 65504 in magnitude (weight " + std::to_string(i) + ")");
        while (flat.size() % 4) flat.push_back(0.f);
        const size_t vr_aligned = flat.size();
        flat.insert(flat.end(), weights + h->Vr, weights + h->Vr + F);
        h->Vr = vr_aligned;
        h->flat.upload(flat);
        h->atom_ids.upload(std::vector<int32_t>(atom_ids, atom_ids + A));
        build_templates(h.get(), edge_src, edge_dst, edge_type);
        h->has_pair = pair_kernel_exists(h->NB, d->precision) && build_pair_template(h.get(), edge_src, edge_dst, edge_type);
        select_template(h.get(), 1 << 20);
        pack_painn(h.get(), weights);
        HIP_CHECK(configure_painn_kernels(h->NB));
        HIP_CHECK(configure_painn_jvp_kernels(h->NB));
        out = h.release();
        return TI_OK;
    });
    return rc == TI_OK ? out : nullptr;
}

int ti_reserve(ti_handle* h, int64_t B)
{
    if (!h || B < 0) return fail(TI_E_ARG, "bad handle / B");
    return guarded([&]() -> int { set_device(h); if (h->kind == 0) ensure_painn_ws(h, B); else ensure_adw_ws(h, B); return TI_OK; });
}

int ti_painn_drift(ti_handle* h, const float* x, float t, const float* cond, int64_t B, float* out, int mem)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (B < 0 || (B > 0 && (!x || !out || (h->ncond > 0 && !cond)))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B);
        ensure_painn_ws(h, B);
        const size_t n = (size_t)B * h->d.n_atoms * 3, nc = (size_t)B * h->d.n_atoms * h->ncond;
        const float *xd = x, *cd = cond; float* od = out;
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(h->x.p, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            if (nc) HIP_CHECK(hipMemcpyAsync(h->cond.p, cond, nc * sizeof(float), hipMemcpyHostToDevice, h->stream));
            xd = h->x.p; cd = h->cond.p; od = h->b1.p;
        }
        painn_drift_dev(h, xd, t, cd, B, od);
        if (mem == TI_MEM_HOST && h->tap < 0) HIP_CHECK(hipMemcpyAsync(out, od, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return TI_OK;
    });
}

int ti_painn_drift_tv(ti_handle* h, const float* x, const float* t, const float* cond, int64_t B, float* out, int mem)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (B < 0 || (B > 0 && (!x || !t || !out || (h->ncond > 0 && !cond)))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B);
        ensure_painn_ws(h, B);
        const size_t n = (size_t)B * h->d.n_atoms * 3, nc = (size_t)B * h->d.n_atoms * h->ncond;
        const float *xd = x, *cd = cond, *td = t; float* od = out;
        if (mem == TI_MEM_HOST) {
            if (h->rk_tv.n < (size_t)B) h->rk_tv.alloc(B);
            HIP_CHECK(hipMemcpyAsync(h->x.p, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            if (nc) HIP_CHECK(hipMemcpyAsync(h->cond.p, cond, nc * sizeof(float), hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(h->rk_tv.p, t, (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
            xd = h->x.p; cd = h->cond.p; td = h->rk_tv.p; od = h->b1.p;
        }
        painn_drift_dev(h, xd, 0.f, cd, B, od, nullptr, td);
        if (mem == TI_MEM_HOST && h->tap < 0) HIP_CHECK(hipMemcpyAsync(out, od, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return TI_OK;
    });
}

int ti_painn_rollout(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* cond, int64_t B, float* out_path,
                     int64_t* n_fevals)
{
    if (int rc = check_rollout_desc(rd)) return rc;          // first: needs no handle
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (rd->scheme == TI_SCHEME_DOPRI5_TRAJ && h->obs[1].K > 0)
        return fail(TI_E_UNSUPPORTED, "TI_SCHEME_DOPRI5_TRAJ writes its rows per trajectory inside a kernel: detach the observer (ti_obs_set_observer)");
    if (B < 0 || (B > 0 && (!x0 || !out_path || (h->ncond > 0 && !cond)))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) { if (n_fevals) *n_fevals = 0; return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B);
        ensure_painn_ws(h, B);
        const int A = h->d.n_atoms;
        const size_t n = (size_t)B * A * 3, nc = (size_t)B * A * h->ncond;
        const hipMemcpyKind in_kind = rd->mem == TI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIP_CHECK(hipMemcpyAsync(h->x.p, x0, n * sizeof(float), in_kind, h->stream));
        const float* cd = cond;
        if (rd->mem == TI_MEM_HOST && nc) { HIP_CHECK(hipMemcpyAsync(h->cond.p, cond, nc * sizeof(float), hipMemcpyHostToDevice, h->stream)); cd = h->cond.p; }
        const int saved_tap = h->tap; h->tap = -1;
        const Ragged rg = ragged_of(h);
        auto drift = [&](const float* xs, float t, float* o, float*) { painn_drift_dev(h, xs, t, cd, B, o); };
        auto drift_tv = [&](const float* xs, const float* tv, float* o, float*) { painn_drift_dev(h, xs, 0.f, cd, B, o, nullptr, tv); };
        const int rc = rd->scheme == TI_SCHEME_DOPRI5_TRAJ ? rollout_rk_traj(h, rd, h->x.p, B, A * 3, out_path, n_fevals, drift_tv, DlogpAux(), rg)
                     : rd->scheme >= TI_SCHEME_DOPRI5 ? rollout_rk(h, rd, h->x.p, n, out_path, n_fevals, drift, DlogpAux(), rg)
                                                      : rollout_common(h, rd, h->x.p, h->b1.p, h->b2.p, h->xt.p, n, B, A * 3, A, out_path, n_fevals, drift, DlogpAux(), rg);
        h->tap = saved_tap;
        return rc;
    });
}

int ti_painn_drift_jvp(ti_handle* h, const float* x, const float* xdot, float t, const float* cond, int64_t B, float* out,
                       float* out_tan, int mem)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->d.precision == TI_PREC_F16) return fail(TI_E_UNSUPPORTED, "the fp16 storage mode has no divergence / tangent path (use f32 or f16x2)");
    if (B < 0 || (B > 0 && (!x || !xdot || !out || !out_tan || (h->ncond > 0 && !cond)))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B, false);
        ensure_painn_ws(h, B);
        ensure_jvp_ws(h, B, 1);
        const size_t n = (size_t)B * h->d.n_atoms * 3, nc = (size_t)B * h->d.n_atoms * h->ncond;
        const float *xd = x, *td = xdot, *cd = cond; float *od = out, *otd = out_tan;
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(h->x.p, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(h->xt.p, xdot, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            if (nc) HIP_CHECK(hipMemcpyAsync(h->cond.p, cond, nc * sizeof(float), hipMemcpyHostToDevice, h->stream));
            xd = h->x.p; td = h->xt.p; cd = h->cond.p; od = h->b1.p; otd = h->tout.p;
        }
        JvpRun jr{1, td, otd};
        painn_drift_dev(h, xd, t, cd, B, od, &jr);
        if (mem == TI_MEM_HOST && h->tap < 0) {
            HIP_CHECK(hipMemcpyAsync(out, od, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipMemcpyAsync(out_tan, otd, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return TI_OK;
    });
}

int ti_painn_drift_div(ti_handle* h, const float* x, float t, const float* cond, int64_t B, float* out, float* out_div, int mem)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->d.precision == TI_PREC_F16) return fail(TI_E_UNSUPPORTED, "the fp16 storage mode has no divergence / tangent path (use f32 or f16x2)");
    if (B < 0 || (B > 0 && (!x || !out || !out_div || (h->ncond > 0 && !cond)))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    if (h->tap >= 0) return fail(TI_E_ARG, "debug taps apply to ti_painn_drift / ti_painn_drift_jvp only");
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B, false);
        ensure_painn_ws(h, B);
        const size_t n = (size_t)B * h->d.n_atoms * 3, nc = (size_t)B * h->d.n_atoms * h->ncond;
        const float *xd = x, *cd = cond; float *od = out, *dd = out_div;
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(h->x.p, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            if (nc) HIP_CHECK(hipMemcpyAsync(h->cond.p, cond, nc * sizeof(float), hipMemcpyHostToDevice, h->stream));
            xd = h->x.p; cd = h->cond.p; od = h->b1.p; dd = h->divb.p;
        }
        painn_drift_div_dev(h, xd, t, cd, B, od, dd);
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(out, od, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipMemcpyAsync(out_div, dd, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return TI_OK;
    });
}

int ti_painn_drift_div_tv(ti_handle* h, const float* x, const float* t, const float* cond, int64_t B, float* out, float* out_div, int mem)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->d.precision == TI_PREC_F16) return fail(TI_E_UNSUPPORTED, "the fp16 storage mode has no divergence / tangent path (use f32 or f16x2)");
    if (B < 0 || (B > 0 && (!x || !t || !out || !out_div || (h->ncond > 0 && !cond)))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    if (h->tap >= 0) return fail(TI_E_ARG, "debug taps apply to ti_painn_drift / ti_painn_drift_jvp only");
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B, false);
        ensure_painn_ws(h, B);
        const size_t n = (size_t)B * h->d.n_atoms * 3, nc = (size_t)B * h->d.n_atoms * h->ncond;
        const float *xd = x, *cd = cond, *td = t; float *od = out, *dd = out_div;
        if (mem == TI_MEM_HOST) {
            if (h->rk_tv.n < (size_t)B) h->rk_tv.alloc(B);
            HIP_CHECK(hipMemcpyAsync(h->x.p, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            if (nc) HIP_CHECK(hipMemcpyAsync(h->cond.p, cond, nc * sizeof(float), hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(h->rk_tv.p, t, (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
            xd = h->x.p; cd = h->cond.p; td = h->rk_tv.p; od = h->b1.p; dd = h->divb.p;
        }
        painn_drift_div_dev(h, xd, 0.f, cd, B, od, dd, td);
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(out, od, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipMemcpyAsync(out_div, dd, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return TI_OK;
    });
}

// ti_painn_rollout_dlogp (n_probes == 0: exact divergence) and ti_painn_rollout_dlogp_est (n_probes >= 1: Hutchinson estimate)
static int painn_rollout_dlogp_impl(ti_handle* h, const ti_rollout_desc* rd, int n_probes, uint64_t probe_seed, const float* x0,
                                    const float* cond, int64_t B, float div_scale, float out_scale, int reverse_ode, float* out_path,
                                    float* out_dlogp, int64_t* n_fevals)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->d.precision == TI_PREC_F16) return fail(TI_E_UNSUPPORTED, "the fp16 storage mode has no divergence / tangent path (use f32 or f16x2)");
    if (int rc = check_rollout_desc(rd)) return rc;
    if (rd->scheme == TI_SCHEME_EM) return fail(TI_E_UNSUPPORTED, "dlogp is defined for the deterministic schemes only (EULER, HEUN)");
    if (rd->scheme == TI_SCHEME_DOPRI5_TRAJ && h->obs[1].K > 0)
        return fail(TI_E_UNSUPPORTED, "TI_SCHEME_DOPRI5_TRAJ writes its rows per trajectory inside a kernel: detach the observer (ti_obs_set_observer)");
    if (B < 0 || (B > 0 && (!x0 || !out_path || !out_dlogp || (h->ncond > 0 && !cond)))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) { if (n_fevals) *n_fevals = 0; return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B, false);
        ensure_painn_ws(h, B);
        const int A = h->d.n_atoms;
        const size_t n = (size_t)B * A * 3, nc = (size_t)B * A * h->ncond;
        const hipMemcpyKind in_kind = rd->mem == TI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIP_CHECK(hipMemcpyAsync(h->x.p, x0, n * sizeof(float), in_kind, h->stream));
        const float* cd = cond;
        if (rd->mem == TI_MEM_HOST && nc) { HIP_CHECK(hipMemcpyAsync(h->cond.p, cond, nc * sizeof(float), hipMemcpyHostToDevice, h->stream)); cd = h->cond.p; }
        const int saved_tap = h->tap; h->tap = -1;
        const Ragged rg = ragged_of(h);
        if (n_probes > 0) painn_make_probes(h, B, n_probes, probe_seed, rd->traj_offset);
        DlogpAux aux;
        aux.dl = h->dl.p; aux.d1 = h->divb.p; aux.d2 = h->div2.p; aux.scaled = h->dlscaled.p; aux.out = out_dlogp;
        aux.n_dl = (size_t)B; aux.div_scale = div_scale; aux.out_scale = out_scale;
        auto drift = [&](const float* xs, float t, float* o, float* dv) {
            if (n_probes > 0) painn_drift_div_est_dev(h, xs, t, cd, B, n_probes, o, dv);
            else painn_drift_div_dev(h, xs, t, cd, B, o, dv);
            if (reverse_ode) {      // (-b, +div): ode_wrapper.py:49
                HIP_CHECK(launch_scale(o, o, -1.0f, (long long)n, h->stream));
                HIP_CHECK(launch_scale(dv, dv, -1.0f, (long long)B, h->stream));
            }
        };
        auto drift_tv = [&](const float* xs, const float* tv, float* o, float* dv) {
            if (n_probes > 0) painn_drift_div_est_dev(h, xs, 0.f, cd, B, n_probes, o, dv, tv);
            else painn_drift_div_dev(h, xs, 0.f, cd, B, o, dv, tv);
            if (reverse_ode) {
                HIP_CHECK(launch_scale(o, o, -1.0f, (long long)n, h->stream));
                HIP_CHECK(launch_scale(dv, dv, -1.0f, (long long)B, h->stream));
            }
        };
        const int rc = rd->scheme == TI_SCHEME_DOPRI5_TRAJ ? rollout_rk_traj(h, rd, h->x.p, B, A * 3, out_path, n_fevals, drift_tv, aux, rg)
                     : rd->scheme >= TI_SCHEME_DOPRI5 ? rollout_rk(h, rd, h->x.p, n, out_path, n_fevals, drift, aux, rg)
                                                      : rollout_common(h, rd, h->x.p, h->b1.p, h->b2.p, h->xt.p, n, B, A * 3, A, out_path, n_fevals, drift, aux, rg);
        h->tap = saved_tap;
        return rc;
    });
}

int ti_painn_rollout_dlogp(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* cond, int64_t B, float div_scale,
                           float out_scale, int reverse_ode, float* out_path, float* out_dlogp, int64_t* n_fevals)
{
    return painn_rollout_dlogp_impl(h, rd, 0, 0, x0, cond, B, div_scale, out_scale, reverse_ode, out_path, out_dlogp, n_fevals);
}

int ti_painn_rollout_dlogp_est(ti_handle* h, const ti_rollout_desc* rd, int32_t n_probes, uint64_t probe_seed, const float* x0,
                               const float* cond, int64_t B, float div_scale, float out_scale, int reverse_ode, float* out_path,
                               float* out_dlogp, int64_t* n_fevals)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->d.precision == TI_PREC_F16) return fail(TI_E_UNSUPPORTED, "the fp16 storage mode has no divergence / tangent path (use f32 or f16x2)");
    if (n_probes < 1) return fail(TI_E_ARG, "n_probes must be >= 1");
    return painn_rollout_dlogp_impl(h, rd, n_probes, probe_seed, x0, cond, B, div_scale, out_scale, reverse_ode, out_path, out_dlogp, n_fevals);
}

// ti_painn_drift_div_est (tv == NULL) / ti_painn_drift_div_est_tv
static int painn_drift_div_est_impl(ti_handle* h, const float* x, float t, const float* tv, const float* cond, int64_t B, int32_t n_probes,
                                    uint64_t probe_seed, int64_t traj_offset, float* out, float* out_div, int mem, bool per_mol_t)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->d.precision == TI_PREC_F16) return fail(TI_E_UNSUPPORTED, "the fp16 storage mode has no divergence / tangent path (use f32 or f16x2)");
    if (n_probes < 1) return fail(TI_E_ARG, "n_probes must be >= 1");
    if (B < 0 || (B > 0 && (!x || (per_mol_t && !tv) || !out || !out_div || (h->ncond > 0 && !cond)))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    if (h->tap >= 0) return fail(TI_E_ARG, "debug taps apply to ti_painn_drift / ti_painn_drift_jvp only");
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B, false);
        ensure_painn_ws(h, B);
        const size_t n = (size_t)B * h->d.n_atoms * 3, nc = (size_t)B * h->d.n_atoms * h->ncond;
        const float *xd = x, *cd = cond, *td = tv; float *od = out, *dd = out_div;
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(h->x.p, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            if (nc) HIP_CHECK(hipMemcpyAsync(h->cond.p, cond, nc * sizeof(float), hipMemcpyHostToDevice, h->stream));
            if (per_mol_t) {
                if (h->rk_tv.n < (size_t)B) h->rk_tv.alloc(B);
                HIP_CHECK(hipMemcpyAsync(h->rk_tv.p, tv, (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
                td = h->rk_tv.p;
            }
            xd = h->x.p; cd = h->cond.p; od = h->b1.p; dd = h->divb.p;
        }
        painn_make_probes(h, B, n_probes, probe_seed, traj_offset);
        painn_drift_div_est_dev(h, xd, t, cd, B, n_probes, od, dd, per_mol_t ? td : nullptr);
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(out, od, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipMemcpyAsync(out_div, dd, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return TI_OK;
    });
}

int ti_painn_drift_div_est(ti_handle* h, const float* x, float t, const float* cond, int64_t B, int32_t n_probes, uint64_t probe_seed,
                           int64_t traj_offset, float* out, float* out_div, int mem)
{
    return painn_drift_div_est_impl(h, x, t, nullptr, cond, B, n_probes, probe_seed, traj_offset, out, out_div, mem, false);
}

int ti_painn_drift_div_est_tv(ti_handle* h, const float* x, const float* t, const float* cond, int64_t B, int32_t n_probes,
                              uint64_t probe_seed, int64_t traj_offset, float* out, float* out_div, int mem)
{
    return painn_drift_div_est_impl(h, x, 0.f, t, cond, B, n_probes, probe_seed, traj_offset, out, out_div, mem, true);
}

int ti_painn_debug_tap(ti_handle* h, int stage)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->d.precision == TI_PREC_F16 && stage >= 0) return fail(TI_E_UNSUPPORTED, "debug taps read fp32 state; not available in the fp16 storage mode");
    h->tap = stage;
    return TI_OK;
}

int ti_painn_debug_poison(ti_handle* h, int64_t B, float value)
{
    if (!h || h->kind != 0 || B <= 0) return fail(TI_E_ARG, "not a painn handle / B");
    return guarded([&]() -> int {
        set_device(h);
        ensure_painn_ws(h, B);
        const size_t N = (size_t)B * h->d.n_atoms, F = h->d.n_features;
        const unsigned bits = __builtin_bit_cast(unsigned, value);
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->dsacc.p, (int)bits, N * F, h->stream));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->dvacc.p, (int)bits, N * 3 * F, h->stream));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->cacc.p, (int)bits, N * 3 * F, h->stream));
        // the edge state and the parked geometry as well: every row a launch reads was written earlier in the same evaluation, and the
        // rows the pair-major kernel skips (pairs that do not exist) are never read
        static_assert(sizeof(*h->e.p) == 4 && sizeof(*h->enc.p) == 4 && sizeof(*h->geo.p) == 4, "32-bit fills");
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->e.p, (int)bits, h->e.n, h->stream));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->enc.p, (int)bits, h->enc.n, h->stream));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->geo.p, (int)bits, h->geo.n, h->stream));
        return TI_OK;
    });
}

int ti_painn_debug_read(ti_handle* h, int what, float* out, size_t n_floats)
{
    if (!h || h->kind != 0 || !out) return fail(TI_E_ARG, "bad argument");
    return guarded([&]() -> int {
        set_device(h);
        const size_t A = h->d.n_atoms, F = h->d.n_features, E = h->d.n_edges, B = (size_t)h->last_B, N = B * A;
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (what == 0) {
            if (n_floats != N * F) return fail(TI_E_ARG, "size mismatch (s)");
            std::vector<float> ds(n_floats);                  // pending invariant messages (zero after an update stage)
            HIP_CHECK(hipMemcpy(out, h->s.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(ds.data(), h->dsacc.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n_floats; ++i) out[i] += ds[i];
        } else if (what == 1) {
            // v as the reference sees it at the tap: v + dvacc + cacc x v (the accumulators are zero after an update stage)
            if (n_floats != N * 3 * F) return fail(TI_E_ARG, "size mismatch (v)");
            std::vector<float> v(n_floats), dv(n_floats), cc(n_floats);
            HIP_CHECK(hipMemcpy(v.data(), h->v.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(dv.data(), h->dvacc.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(cc.data(), h->cacc.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t nd = 0; nd < N; ++nd)
                for (size_t f = 0; f < F; ++f)
                    for (int c = 0; c < 3; ++c) {
                        const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                        auto at = [&](const std::vector<float>& a, int cc2) { return a[(nd * 3 + cc2) * F + f]; };
                        out[(nd * 3 + c) * F + f] = (at(v, c) + at(dv, c)) + (at(cc, c1) * at(v, c2) - at(cc, c2) * at(v, c1));
                    }
        } else if (what == 2) {
            if (n_floats != B * E * F) return fail(TI_E_ARG, "size mismatch (e)");
            const size_t RB = ti::EDGE_ROWS_PER_BLOCK, rows = (B + h->G - 1) / h->G * h->parts * h->nblk * RB * (h->active == 2 ? 2 : 1);
            std::vector<float> e(rows * F);
            HIP_CHECK(hipMemcpy(e.data(), h->e.p, e.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t m = 0; m < B; ++m)
                for (size_t k = 0; k < E; ++k)                                   // k = sorted position
                    std::memcpy(out + (m * E + h->perm[k]) * F, e.data() + edge_row_of(h, m, k) * F, F * sizeof(float));
        } else if (what >= 3 && what <= 5) {
            // tangents of the last ti_painn_drift_jvp call (one direction per molecule), composed like their primal twins
            if (h->last_D != 1 || (size_t)h->last_VB != B) return fail(TI_E_ARG, "tangent taps need a preceding ti_painn_drift_jvp call");
            auto fetch = [&](const DevBuf<float>& b, size_t n) { std::vector<float> v(n); HIP_CHECK(hipMemcpy(v.data(), b.p, n * sizeof(float), hipMemcpyDeviceToHost)); return v; };
            if (what == 3) {
                if (n_floats != N * F) return fail(TI_E_ARG, "size mismatch (ts)");
                const auto ts = fetch(h->ts, n_floats), td = fetch(h->tdsacc, n_floats);
                for (size_t i = 0; i < n_floats; ++i) out[i] = ts[i] + td[i];
            } else if (what == 4) {
                if (n_floats != N * 3 * F) return fail(TI_E_ARG, "size mismatch (tv)");
                const auto v = fetch(h->v, n_floats), cc = fetch(h->cacc, n_floats);
                const auto tv = fetch(h->tv, n_floats), tdv = fetch(h->tdvacc, n_floats), tcc = fetch(h->tcacc, n_floats);
                for (size_t nd = 0; nd < N; ++nd)
                    for (size_t f = 0; f < F; ++f)
                        for (int c = 0; c < 3; ++c) {
                            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                            auto at = [&](const std::vector<float>& a, int cc2) { return a[(nd * 3 + cc2) * F + f]; };
                            out[(nd * 3 + c) * F + f] = (at(tv, c) + at(tdv, c)) + ((at(tcc, c1) * at(v, c2) + at(cc, c1) * at(tv, c2)) -
                                                                                     (at(tcc, c2) * at(v, c1) + at(cc, c2) * at(tv, c1)));
                        }
            } else {
                if (n_floats != B * E * F) return fail(TI_E_ARG, "size mismatch (te)");
                const size_t RB = ti::EDGE_ROWS_PER_BLOCK, rows = (B + h->G - 1) / h->G * h->parts * h->nblk * RB;
                const auto e = fetch(h->te, rows * F);
                for (size_t m = 0; m < B; ++m)
                    for (size_t k = 0; k < E; ++k)
                        std::memcpy(out + (m * E + h->perm[k]) * F, e.data() + edge_row_of(h, m, k) * F, F * sizeof(float));
            }
        } else return fail(TI_E_ARG, "unknown tap");
        return TI_OK;
    });
}

// ------------------------------------------------------------------------------------------------------------ adw
ti_handle* ti_adw_create(const ti_adw_desc* d, const double* weights, size_t n_weights, int device)
{
    return ti_adw_create_nd(d, 1, weights, n_weights, device);
}

ti_handle* ti_adw_create_nd(const ti_adw_desc* d, int32_t dim, const double* weights, size_t n_weights, int device)
{
    ti_handle* out = nullptr;
    const int rc = guarded([&]() -> int {
        if (!d || !weights) return fail(TI_E_ARG, "NULL argument");
        if (dim < 1 || dim > 16) return fail(TI_E_UNSUPPORTED, "dim must be 1..16 (FCNetMultiBeta(d, d, H, L)), got " + std::to_string(dim));
        const int H = d->hidden_size, nl = d->num_layers;
        if (H != 32 && H != 64 && H != 128 && H != 256) return fail(TI_E_UNSUPPORTED, "hidden_size must be 32, 64, 128 or 256");
        if (nl < 1) return fail(TI_E_ARG, "num_layers must be >= 1");
        if (d->precision != TI_PREC_F32 && d->precision != TI_PREC_F16X2) return fail(TI_E_ARG, "unknown precision");
        const size_t need = (size_t)H * 3 + H + (size_t)H * H + H + H + 1 + (size_t)H * (dim + 2) + H + (size_t)(nl - 1) * ((size_t)H * H + H) +
                            (size_t)dim * H + dim;
        if (n_weights != need) return fail(TI_E_ARG, "weight count mismatch: expected " + std::to_string(need) + ", got " + std::to_string(n_weights));
        std::unique_ptr<ti_handle> h(new_handle(1, device));
        h->ad = *d; h->NB = H / 32; h->a_dim = dim;
        std::vector<float> w(n_weights);
        for (size_t i = 0; i < n_weights; ++i) w[i] = (float)weights[i];        // the device computes in fp32
        const int NB = h->NB, NBK = H / 16;
        const bool split = d->precision == TI_PREC_F16X2;
        std::vector<float> nat, pk;
        auto chunk16 = [&](const float* W, int row0) {
            if (split) pack_chunk16_split(pk, W, H, H, row0, 0, NBK); else pack_chunk16(pk, W, H, H, row0, 0, NBK);
        };
        // one MLP block: canonical order  W_in[H,K] b_in[H] (W_h[H,H] b_h[H]) x n_hidden  W_out[D,H] b_out[D]  (K = D + 2)
        // D = 1: vector block w_in [H][3] | b_in | b_hidden | w_out, b_out a kernel argument.  D > 1: w_in [H][Kpad] (zero
        // columns up to a multiple of 4) | b_in | b_hidden | w_out [D][H] | b_out [D] (zeros up to a multiple of 4).
        auto take_mlp = [&](size_t& o, int n_hidden, size_t& vec_off, Stream& st, float& b_out, int D) {
            vec_off = nat.size();
            const int K = D + 2, Kpad = D == 1 ? 3 : (K + 3) / 4 * 4;
            for (int f = 0; f < H; ++f) {                                               // w_in
                nat.insert(nat.end(), &w[o + (size_t)f * K], &w[o + (size_t)f * K] + K);
                nat.insert(nat.end(), (size_t)(Kpad - K), 0.f);
            }
            o += (size_t)H * K;
            nat.insert(nat.end(), &w[o], &w[o] + H); o += H;                              // b_in
            st.off4 = pk.size() / 4;
            std::vector<float> bh;
            for (int l = 0; l < n_hidden; ++l) {
                for (int nbo = 0; nbo < NB; ++nbo) chunk16(&w[o], 32 * nbo);
                o += (size_t)H * H;
                bh.insert(bh.end(), &w[o], &w[o] + H); o += H;
            }
            st.nch = n_hidden * NB;
            nat.insert(nat.end(), bh.begin(), bh.end());
            nat.insert(nat.end(), &w[o], &w[o] + (size_t)D * H); o += (size_t)D * H;      // w_out
            if (D == 1) { b_out = w[o]; o += 1; return; }
            nat.insert(nat.end(), &w[o], &w[o] + D); o += D;                               // b_out
            nat.insert(nat.end(), (size_t)((D + 3) / 4 * 4 - D), 0.f);
            b_out = 0.f;
        };
        size_t o = 0;
        take_mlp(o, 1, h->a_be_vecs, h->st_be, h->a_be_b_out, 1);
        take_mlp(o, nl - 1, h->a_net_vecs, h->st_net, h->a_b_out, dim);
        if (pk.empty()) pk.assign(4, 0.f);
        h->flat.upload(nat); h->packed.upload(pk);
        HIP_CHECK(configure_adw_kernels(NB, std::max(1, nl - 1), dim));
        if (dim == 1) HIP_CHECK(configure_adw_fused_kernels(NB, std::max(1, nl - 1)));
        out = h.release();
        return TI_OK;
    });
    return rc == TI_OK ? out : nullptr;
}

static int adw_drift_impl(ti_handle* h, const float* x, float t, const float* beta0, const float* beta1, int64_t B, float* out,
                          float* out_div, int mem)
{
    if (!h || h->kind != 1) return fail(TI_E_ARG, "not an adw handle");
    if (B < 0 || (B > 0 && (!x || !beta0 || !beta1 || !out))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        ensure_adw_ws(h, B);
        const long long U = adw_set_cond(h, beta0, beta1, B, mem);
        const float* xd = x; float* od = out; float* dd = out_div;
        const size_t n = (size_t)B * h->a_dim;
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(h->ax.p, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            xd = h->ax.p; od = h->ab1.p; dd = out_div ? h->ad1.p : nullptr;
        }
        adw_drift_dev(h, xd, t, U, B, od, dd);
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(out, od, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            if (out_div) HIP_CHECK(hipMemcpyAsync(out_div, dd, B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return TI_OK;
    });
}

int ti_adw_drift(ti_handle* h, const float* x, float t, const float* beta0, const float* beta1, int64_t B, float* out, int mem)
{
    return adw_drift_impl(h, x, t, beta0, beta1, B, out, nullptr, mem);
}

int ti_adw_drift_div(ti_handle* h, const float* x, float t, const float* beta0, const float* beta1, int64_t B, float* out, float* out_div, int mem)
{
    if (!out_div) return fail(TI_E_ARG, "out_div is NULL");
    return adw_drift_impl(h, x, t, beta0, beta1, B, out, out_div, mem);
}

int ti_adw_drift_tv(ti_handle* h, const float* x, const float* t, const float* beta0, const float* beta1, int64_t B, float* out,
                    float* out_div, int mem)
{
    if (!h || h->kind != 1) return fail(TI_E_ARG, "not an adw handle");
    if (B < 0 || (B > 0 && (!x || !t || !beta0 || !beta1 || !out))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        ensure_adw_ws(h, B);
        const float *b0d = nullptr, *b1d = nullptr;
        adw_rows_dev(h, beta0, beta1, B, mem, &b0d, &b1d);
        const float *xd = x, *td = t; float* od = out; float* dd = out_div;
        const size_t n = (size_t)B * h->a_dim;
        if (mem == TI_MEM_HOST) {
            if (h->atv.n < (size_t)B) h->atv.alloc(B);
            HIP_CHECK(hipMemcpyAsync(h->ax.p, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(h->atv.p, t, B * sizeof(float), hipMemcpyHostToDevice, h->stream));
            xd = h->ax.p; td = h->atv.p; od = h->ab1.p; dd = out_div ? h->ad1.p : nullptr;
        }
        adw_drift_tv_dev(h, xd, td, b0d, b1d, B, od, dd);
        if (mem == TI_MEM_HOST) {
            HIP_CHECK(hipMemcpyAsync(out, od, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            if (out_div) HIP_CHECK(hipMemcpyAsync(out_div, dd, B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return TI_OK;
    });
}

static int adw_rollout_impl(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* beta0, const float* beta1, int64_t B,
                            float* out_path, float* out_dlogp, int64_t* n_fevals)
{
    if (!h || h->kind != 1) return fail(TI_E_ARG, "not an adw handle");
    if (int rc = check_rollout_desc(rd)) return rc;
    if (rd->scheme == TI_SCHEME_DOPRI5_TRAJ && h->obs[1].K > 0)
        return fail(TI_E_UNSUPPORTED, "TI_SCHEME_DOPRI5_TRAJ writes its rows per trajectory inside a kernel: detach the observer (ti_obs_set_observer)");
    if (B < 0 || (B > 0 && (!x0 || !beta0 || !beta1 || !out_path))) return fail(TI_E_ARG, "NULL buffer");
    if (out_dlogp && rd->scheme == TI_SCHEME_EM && rd->eps > 0.f)
        return fail(TI_E_UNSUPPORTED, "dlogp is defined for a deterministic flow: EM needs eps = 0");
    if (B == 0) { if (n_fevals) *n_fevals = 0; return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        ensure_adw_ws(h, B);
        const long long U = adw_set_cond(h, beta0, beta1, B, rd->mem);
        const hipMemcpyKind in_kind = rd->mem == TI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        const int D = h->a_dim;
        const size_t n = (size_t)B * D;
        HIP_CHECK(hipMemcpyAsync(h->ax.p, x0, n * sizeof(float), in_kind, h->stream));
        DlogpAux aux;
        aux.n_dl = (size_t)B;                        // one dlogp entry per particle
        DevBuf<float> scaled_tmp;                    // dlogp * 1e2 staging for the saved rows
        if (out_dlogp) { scaled_tmp.alloc(B); aux.dl = h->adl.p; aux.d1 = h->ad1.p; aux.d2 = h->ad2.p; aux.scaled = scaled_tmp.p; aux.out = out_dlogp; }
        auto drift = [&](const float* xs, float t, float* o, float* dv) { adw_drift_dev(h, xs, t, U, B, o, dv); };
        if (rd->scheme == TI_SCHEME_DOPRI5_TRAJ) {
            const float *b0d = nullptr, *b1d = nullptr;
            adw_rows_dev(h, beta0, beta1, B, rd->mem, &b0d, &b1d);
            auto drift_tv = [&](const float* xs, const float* tv, float* o, float* dv) { adw_drift_tv_dev(h, xs, tv, b0d, b1d, B, o, dv); };
            return rollout_rk_traj(h, rd, h->ax.p, B, D, out_path, n_fevals, drift_tv, aux);
        }
        if (rd->scheme >= TI_SCHEME_DOPRI5) return rollout_rk(h, rd, h->ax.p, n, out_path, n_fevals, drift, aux);
        return rollout_common(h, rd, h->ax.p, h->ab1.p, h->ab2.p, h->axt.p, n, B, D, 0, out_path, n_fevals, drift, aux);
    });
}

int ti_adw_rollout(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* beta0, const float* beta1, int64_t B,
                   float* out_path, int64_t* n_fevals)
{
    return adw_rollout_impl(h, rd, x0, beta0, beta1, B, out_path, nullptr, n_fevals);
}

int ti_adw_rollout_dlogp(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* beta0, const float* beta1, int64_t B,
                         float* out_path, float* out_dlogp, int64_t* n_fevals)
{
    if (!out_dlogp) return fail(TI_E_ARG, "out_dlogp is NULL");
    return adw_rollout_impl(h, rd, x0, beta0, beta1, B, out_path, out_dlogp, n_fevals);
}

// A whole Euler / Heun / EM rollout of a 1-D handle in two launches: the beta-embedding table of every grid point (the embedding
// kernel in its per-row-time mode over n_step * U rows) and adw_rollout_fused_kernel.  Every per-step scalar is computed here with the
// fp32 expressions of rollout_common; the kernel applies them with the roundings of axpy_kernel / heun_kernel / noise_kernel /
// scale_kernel, so the result is that of ti_adw_rollout(_dlogp) bit for bit.
int ti_adw_rollout_fused(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* beta0, const float* beta1, int64_t B,
                         float* out_path, float* out_dlogp, int64_t* n_fevals)
{
    if (!h || h->kind != 1) return fail(TI_E_ARG, "not an adw handle");
    if (int rc = check_rollout_desc(rd)) return rc;
    if (h->a_dim > 1) return fail(TI_E_UNSUPPORTED, "the fused rollout covers 1-D handles: use ti_adw_rollout for dim = " + std::to_string(h->a_dim));
    if (rd->scheme != TI_SCHEME_EULER && rd->scheme != TI_SCHEME_HEUN && rd->scheme != TI_SCHEME_EM)
        return fail(TI_E_UNSUPPORTED, "the fused rollout covers the Euler, Heun and EM schemes: use ti_adw_rollout for the others");
    if (h->obs[1].K > 0)
        return fail(TI_E_UNSUPPORTED, "the fused rollout writes its rows inside a kernel: detach the observer (ti_obs_set_observer)");
    if (B < 0 || (B > 0 && (!x0 || !beta0 || !beta1 || !out_path))) return fail(TI_E_ARG, "NULL buffer");
    if (out_dlogp && rd->scheme == TI_SCHEME_EM && rd->eps > 0.f)
        return fail(TI_E_UNSUPPORTED, "dlogp is defined for a deterministic flow: EM needs eps = 0");
    if (B == 0) { if (n_fevals) *n_fevals = 0; return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        ensure_adw_ws(h, B);
        std::vector<float> u0, u1;
        const long long U = adw_set_cond(h, beta0, beta1, B, rd->mem, &u0, &u1);
        const int N = rd->n_step;
        if ((long long)N * U > (1LL << 24))
            return fail(TI_E_UNSUPPORTED, "the fused rollout's embedding table is limited to 2^24 rows, n_step * distinct (beta0, beta1) pairs = " +
                                              std::to_string((long long)N * U) + ": use ti_adw_rollout");
        hipStream_t st = h->stream;
        const bool dev = rd->mem == TI_MEM_DEVICE;
        HIP_CHECK(hipMemcpyAsync(h->ax.p, x0, (size_t)B * sizeof(float), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        // beta embedding at every grid point, rows (k, u): one launch of the embedding kernel with one time per row
        const size_t nt = (size_t)N * U;
        std::vector<float> tb0(nt), tb1(nt), ttv(nt);
        for (int k = 0; k < N; ++k)
            for (long long u = 0; u < U; ++u) { tb0[k * U + u] = u0[u]; tb1[k * U + u] = u1[u]; ttv[k * U + u] = rd->t_grid[k]; }
        // (the host vectors of this call outlive the stream synchronisation at its end)
        if (h->af_emb.n < nt) { h->af_b0.alloc(nt); h->af_b1.alloc(nt); h->af_tv.alloc(nt); h->af_emb.alloc(nt); }
        HIP_CHECK(hipMemcpyAsync(h->af_b0.p, tb0.data(), nt * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(h->af_b1.p, tb1.data(), nt * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(h->af_tv.p, ttv.data(), nt * sizeof(float), hipMemcpyHostToDevice, st));
        adw_mlp_launch(h, true, h->af_b0.p, h->af_b1.p, h->af_tv.p, nullptr, 0.f, (long long)nt, h->af_emb.p, nullptr);
        // per-step scalars: the expressions of rollout_common, in fp32
        const DlogpAux aux;
        const bool noise = rd->scheme == TI_SCHEME_EM && rd->eps > 0.0f;
        std::vector<AdwFusedStep> steps(std::max(N - 1, 1));
        for (int k = 0; k < N - 1; ++k) {
            const float dt = rd->t_grid[k + 1] - rd->t_grid[k];
            AdwFusedStep& s = steps[k];
            s.t = rd->t_grid[k]; s.t_next = rd->t_grid[k + 1];
            s.dt = dt; s.hdt = 0.5f * dt;
            s.ndt = -dt * aux.div_scale; s.nhdt = -0.5f * dt * aux.div_scale;
            s.sigma = noise ? std::sqrt(2.0f * rd->eps * std::fabs(dt)) : 0.0f;
            s.pad = 0.0f;
        }
        if (h->af_steps.n < steps.size()) h->af_steps.alloc(steps.size());
        HIP_CHECK(hipMemcpyAsync(h->af_steps.p, steps.data(), steps.size() * sizeof(AdwFusedStep), hipMemcpyHostToDevice, st));
        const size_t rows = (size_t)ti_rollout_rows(N, rd->save_every), nout = rows * (size_t)B;
        float *pd = out_path, *dd = out_dlogp;
        if (!dev) {
            if (h->af_path.n < nout) h->af_path.alloc(nout);
            pd = h->af_path.p;
            if (out_dlogp) { if (h->af_dl.n < nout) h->af_dl.alloc(nout); dd = h->af_dl.p; }
        }
        AdwFusedParams p{};
        p.stream = h->S(h->st_net); p.nch = h->st_net.nch; p.vecs = h->F(h->a_net_vecs); p.b_out = h->a_b_out;
        p.n_hidden = h->ad.num_layers - 1; p.B = B;
        p.x = h->ax.p; p.idx = h->aidx.p; p.emb = h->af_emb.p; p.U = U; p.steps = h->af_steps.p;
        p.n_step = N; p.save_every = rd->save_every;
        p.scheme = rd->scheme == TI_SCHEME_HEUN ? ADW_FUSED_HEUN : noise ? ADW_FUSED_EM : ADW_FUSED_EULER;
        p.seed = rd->seed; p.traj0 = rd->traj_offset; p.step0 = (int)rd->step_offset;
        p.out_path = pd; p.out_dlogp = dd; p.out_scale = aux.out_scale;
        {
            Timed tm(h, TI_KERNEL_ADW);
            HIP_CHECK(launch_adw_fused(h->NB, h->ad.precision == TI_PREC_F16X2, p, st));
        }
        if (!dev) {
            HIP_CHECK(hipMemcpyAsync(out_path, pd, nout * sizeof(float), hipMemcpyDeviceToHost, st));
            if (out_dlogp) HIP_CHECK(hipMemcpyAsync(out_dlogp, dd, nout * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipMemsetAsync(h->nanflag.p, 0, sizeof(int), st));
        HIP_CHECK(launch_nan_check(h->ax.p, (long long)B, h->nanflag.p, st));
        int flag = 0;
        HIP_CHECK(hipMemcpyAsync(&flag, h->nanflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (n_fevals) *n_fevals = (int64_t)(N - 1) * (rd->scheme == TI_SCHEME_HEUN ? 2 : 1);
        return flag ? fail(TI_E_NAN, "non-finite value in the final state") : TI_OK;
    });
}

// ---------------------------------------------------------------------------------------------------- observables
int ti_obs_cv(ti_handle* h, const int32_t* desc, int32_t K, const float* ref, const int32_t* select, const float* x, int64_t B,
              float* out_cv, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (!desc) return fail(TI_E_ARG, "desc is NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (B < 0 || (B > 0 && (!x || !out_cv))) return fail(TI_E_ARG, "NULL buffer");
    return guarded([&]() -> int {
        if (int rc = obs_upload(h, 0, desc, K, ref, select)) return rc;
        if (B == 0) return TI_OK;
        const size_t n = (size_t)B * obs_floats_per_traj(h), nk = (size_t)B * K;
        const float* xd = x; float* od = out_cv;
        if (mem == TI_MEM_HOST) {
            if (h->obs_x.n < n) h->obs_x.alloc(n);
            if (h->obs_cv.n < nk) h->obs_cv.alloc(nk);
            HIP_CHECK(hipMemcpyAsync(h->obs_x.p, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
            xd = h->obs_x.p; od = h->obs_cv.p;
        }
        obs_cv_dev(h, 0, xd, B, od);
        if (mem == TI_MEM_HOST) HIP_CHECK(hipMemcpyAsync(out_cv, od, nk * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return TI_OK;
    });
}

// (max, first bad index, sum w, sum w^2) of logw_dev into h->obs_red[0..3] and `norm`; TI_E_NAN on a non-finite entry
static int obs_norm_dev(ti_handle* h, const float* logw_dev, long long B, double norm[4])
{
    hipStream_t st = h->stream;
    if (h->obs_red.n < 4 + 259) h->obs_red.alloc(4 + 259);
    if (h->obs_part.n < (size_t)OBS_MAX_BLOCKS * 259) h->obs_part.alloc((size_t)OBS_MAX_BLOCKS * 259);
    HIP_CHECK(launch_obs_logw_max(h->obs_red.p, h->obs_part.p, logw_dev, B, st));
    HIP_CHECK(hipMemcpyAsync(norm, h->obs_red.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (norm[1] < (double)B) return fail(TI_E_NAN, "non-finite logw at index " + std::to_string((long long)norm[1]));
    HIP_CHECK(launch_obs_logw_sums(h->obs_red.p + 2, h->obs_part.p, logw_dev, h->obs_red.p, B, st));
    HIP_CHECK(hipMemcpyAsync(norm + 2, h->obs_red.p + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    // the kernels that follow read (max, sum w) as one pair
    HIP_CHECK(hipMemcpyAsync(h->obs_red.p + 1, h->obs_red.p + 2, sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return TI_OK;
}

int ti_obs_weights(ti_handle* h, const float* logw, int64_t B, float* out_w, double* out_ess, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (B < 1) return fail(TI_E_ARG, "B < 1");
    if (!logw || !out_ess) return fail(TI_E_ARG, "NULL buffer");
    return guarded([&]() -> int {
        set_device(h);
        const float* ld = logw; float* wd = out_w;
        if (mem == TI_MEM_HOST) {
            if (h->obs_logw.n < (size_t)B) h->obs_logw.alloc(B);
            HIP_CHECK(hipMemcpyAsync(h->obs_logw.p, logw, (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
            ld = h->obs_logw.p;
            if (out_w) { if (h->obs_w.n < (size_t)B) h->obs_w.alloc(B); wd = h->obs_w.p; }
        }
        double norm[4];
        if (int rc = obs_norm_dev(h, ld, B, norm)) return rc;
        *out_ess = norm[2] * norm[2] / norm[3];
        if (out_w) {
            HIP_CHECK(launch_obs_weights(wd, ld, h->obs_red.p, B, h->stream));
            if (mem == TI_MEM_HOST) HIP_CHECK(hipMemcpyAsync(out_w, wd, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        return TI_OK;
    });
}

int ti_obs_hist(ti_handle* h, const float* values, int64_t stride, const float* logw, int64_t B, int32_t n_bins, double lo, double hi,
                double* out_hist, double* out_tails, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n_bins < 1 || n_bins > 256) return fail(TI_E_ARG, "n_bins must be in 1..256");
    if (!(hi > lo) || !std::isfinite(lo) || !std::isfinite(hi)) return fail(TI_E_ARG, "the range needs finite lo < hi");
    if (B < 1 || stride < 1) return fail(TI_E_ARG, "B < 1 or stride < 1");
    if (!values || !out_hist || !out_tails) return fail(TI_E_ARG, "NULL buffer");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const float *vd = values, *ld = logw;
        long long sd = stride;
        if (mem == TI_MEM_HOST) {                      // the column only: B floats, not B * stride
            if (h->obs_val.n < (size_t)B) h->obs_val.alloc(B);
            std::vector<float> col((size_t)B);
            for (int64_t i = 0; i < B; ++i) col[i] = values[i * stride];
            HIP_CHECK(hipMemcpy(h->obs_val.p, col.data(), (size_t)B * sizeof(float), hipMemcpyHostToDevice));
            vd = h->obs_val.p; sd = 1;
            if (logw) {
                if (h->obs_logw.n < (size_t)B) h->obs_logw.alloc(B);
                HIP_CHECK(hipMemcpyAsync(h->obs_logw.p, logw, (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
                ld = h->obs_logw.p;
            }
        }
        double norm[4];
        if (logw) { if (int rc = obs_norm_dev(h, ld, B, norm)) return rc; }
        else {
            if (h->obs_red.n < 4 + 259) h->obs_red.alloc(4 + 259);
            if (h->obs_part.n < (size_t)OBS_MAX_BLOCKS * 259) h->obs_part.alloc((size_t)OBS_MAX_BLOCKS * 259);
        }
        HIP_CHECK(launch_obs_whist(h->obs_red.p + 4, h->obs_part.p, vd, sd, ld, h->obs_red.p, B, n_bins, lo, hi, st));
        std::vector<double> out((size_t)n_bins + 3);
        HIP_CHECK(hipMemcpyAsync(out.data(), h->obs_red.p + 4, out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::copy(out.begin(), out.begin() + n_bins, out_hist);
        std::copy(out.begin() + n_bins, out.end(), out_tails);
        return TI_OK;
    });
}

int ti_obs_set_observer(ti_handle* h, const int32_t* desc, int32_t K, const float* ref, const int32_t* select, int32_t every,
                        float* out_cv, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (!desc) { h->obs[1].K = 0; h->obs_out = nullptr; return TI_OK; }
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (every < 0) return fail(TI_E_ARG, "every must be >= 0");
    if (!out_cv) return fail(TI_E_ARG, "out_cv is NULL");
    return guarded([&]() -> int {
        if (int rc = obs_upload(h, 1, desc, K, ref, select)) return rc;
        h->obs_every = every; h->obs_mem = mem; h->obs_out = out_cv;
        return TI_OK;
    });
}

// --------------------------------------------------------------------------------------------------------- shared
int ti_rollout_step_counts(ti_handle* h, int64_t* accepted, int64_t* rejected, int64_t B)
{
    if (!h || !accepted || !rejected) return fail(TI_E_ARG, "NULL argument");
    if (B != (int64_t)h->traj_accepted.size())
        return fail(TI_E_ARG, "B = " + std::to_string(B) + " does not match the last per-trajectory rollout (" + std::to_string(h->traj_accepted.size()) + " trajectories)");
    std::copy(h->traj_accepted.begin(), h->traj_accepted.end(), accepted);
    std::copy(h->traj_rejected.begin(), h->traj_rejected.end(), rejected);
    return TI_OK;
}

void ti_destroy(ti_handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

int ti_set_stream(ti_handle* h, void* hip_stream, int mode)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (mode != TI_STREAM_OWN && mode != TI_STREAM_EXTERNAL) return fail(TI_E_ARG, "unknown stream mode");
    h->stream = mode == TI_STREAM_EXTERNAL ? reinterpret_cast<hipStream_t>(hip_stream) : h->own_stream;
    return TI_OK;
}

int ti_wait_stream(ti_handle* h, void* producer_stream)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t prod = reinterpret_cast<hipStream_t>(producer_stream);
        if (prod == h->stream) return TI_OK;                     // same stream: already ordered
        if (!h->wait_ev) HIP_CHECK(hipEventCreateWithFlags(&h->wait_ev, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(h->wait_ev, prod));
        HIP_CHECK(hipStreamWaitEvent(h->stream, h->wait_ev, 0));
        return TI_OK;
    });
}

int ti_painn_set_template(ti_handle* h, int which)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (which != TI_TEMPLATE_AUTO && which != TI_TEMPLATE_THROUGHPUT && which != TI_TEMPLATE_LATENCY && which != TI_TEMPLATE_PAIR) return fail(TI_E_ARG, "unknown template");
    if (which == TI_TEMPLATE_LATENCY && h->n_tpl < 2) which = TI_TEMPLATE_THROUGHPUT;      // this species has only one layout
    if (which == TI_TEMPLATE_PAIR && !h->has_pair) which = TI_TEMPLATE_THROUGHPUT;         // no pair-major layout for this graph / width / precision
    h->pinned_tpl = which;
    return TI_OK;
}

int ti_painn_template_for(ti_handle* h, int64_t B)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->has_pair && mask_blocks_pair(h) && pinned_template(h) == TI_TEMPLATE_PAIR)
        return fail(TI_E_UNSUPPORTED, "the pair layout is pinned, and the edge mask in force is not symmetric for every molecule");
    return template_for(h, B);
}

// The per-molecule graph state both setters below write: mask m [B][A] (bits of pad atoms cleared here), atom counts (empty: all A),
// edge types (empty: the template's).  Replaces whatever was in force.
static int set_graph_state(ti_handle* h, std::vector<uint32_t>& m, std::vector<int32_t>& natoms, std::vector<uint8_t>& ptype, long long B)
{
    const int A = h->d.n_atoms;
    long long n_real = (long long)B * A; bool ragged = false;
    if (!natoms.empty()) {
        n_real = 0;
        for (long long b = 0; b < B; ++b) {
            const int n = natoms[b];
            n_real += n; ragged = ragged || n < A;
            const uint32_t real = n >= 32 ? 0xffffffffu : (1u << n) - 1u;         // sources that are real atoms
            for (int d = 0; d < A; ++d) m[(size_t)b * A + d] = d < n ? m[(size_t)b * A + d] & real : 0u;
        }
    }
    // symmetric over the template: for every template edge s -> d whose reverse is one too, both bits (and, where the edge is present,
    // both types) agree in every molecule
    std::vector<uint32_t> in_tpl(A, 0);          // bit s of in_tpl[d]: s -> d is a template edge
    for (size_t k = 0; k < h->esrc.size(); ++k) in_tpl[h->edst[k]] |= 1u << h->esrc[k];
    bool sym = true;
    for (long long b = 0; b < B && sym; ++b)
        for (int d = 0; d < A && sym; ++d)
            for (int s2 = 0; s2 < A; ++s2) {
                if (!((in_tpl[d] >> s2) & 1u) || !((in_tpl[s2] >> d) & 1u)) continue;
                const uint32_t on = (m[(size_t)b * A + d] >> s2) & 1u;
                if (on != ((m[(size_t)b * A + s2] >> d) & 1u)) { sym = false; break; }
                if (on && !ptype.empty() && ptype[((size_t)b * A + s2) * A + d] != ptype[((size_t)b * A + d) * A + s2]) { sym = false; break; }
            }
    if (h->emask_B == B && m == h->emask && natoms == h->natoms && ptype == h->ptype) return TI_OK;      // the same state again (a mirror class sets it before every call)
    HIP_CHECK(hipStreamSynchronize(h->stream));                   // no launch in flight still reads the row words about to be replaced
    h->emask.swap(m); h->emask_B = B; h->emask_sym = sym;
    h->natoms.swap(natoms); h->ptype.swap(ptype); h->ragged = ragged; h->n_real = n_real;
    if (ragged) h->natoms_dev.upload(h->natoms); else h->natoms_dev.release();
    for (int t = 0; t < 3; ++t) h->mrows_ok[t] = false;
    return TI_OK;
}

static void clear_graph_state(ti_handle* h)
{
    h->emask_B = 0; h->emask_sym = true; h->emask.clear(); h->natoms.clear(); h->ptype.clear(); h->ragged = false; h->n_real = 0;
    for (int t = 0; t < 3; ++t) { h->mrows_ok[t] = false; h->mrows[t].release(); }
}

int ti_painn_set_edge_mask(ti_handle* h, const uint32_t* mask, int64_t B, int mem)
{
    // the arguments first, then the handle: each refusal has its own message, checkable without a device
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (mask && B < 1) return fail(TI_E_ARG, "B < 1");
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (!mask) { clear_graph_state(h); return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        const int A = h->d.n_atoms;
        std::vector<uint32_t> m((size_t)B * A);
        if (mem == TI_MEM_DEVICE) HIP_CHECK(hipMemcpy(m.data(), mask, m.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        else std::memcpy(m.data(), mask, m.size() * sizeof(uint32_t));
        std::vector<int32_t> none; std::vector<uint8_t> no_types;
        return set_graph_state(h, m, none, no_types, B);
    });
}

int ti_painn_set_molecules(ti_handle* h, const int32_t* n_atoms, const uint32_t* mask, const uint8_t* pair_type, int64_t B, int mem)
{
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n_atoms && B < 1) return fail(TI_E_ARG, "B < 1");
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (!n_atoms) { clear_graph_state(h); return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        const int A = h->d.n_atoms;
        auto fetch = [&](void* dst, const void* src, size_t bytes) {
            if (mem == TI_MEM_DEVICE) HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            else std::memcpy(dst, src, bytes);
        };
        std::vector<int32_t> na((size_t)B);
        fetch(na.data(), n_atoms, na.size() * sizeof(int32_t));
        for (long long b = 0; b < B; ++b)
            if (na[b] < 1 || na[b] > A) return fail(TI_E_ARG, "n_atoms[" + std::to_string(b) + "] = " + std::to_string(na[b]) + " is outside 1.." + std::to_string(A));
        std::vector<uint8_t> pt;
        if (pair_type) {
            pt.resize((size_t)B * A * A);
            fetch(pt.data(), pair_type, pt.size());
            for (size_t i = 0; i < pt.size(); ++i) if (pt[i] > 3) return fail(TI_E_ARG, "pair_type above 3 (molecule " + std::to_string(i / ((size_t)A * A)) + ")");
        }
        std::vector<uint32_t> m((size_t)B * A, 0xffffffffu);       // NULL: every template edge (between real atoms, set_graph_state)
        if (mask) fetch(m.data(), mask, m.size() * sizeof(uint32_t));
        return set_graph_state(h, m, na, pt, B);
    });
}

int ti_profile_enable(ti_handle* h, int on)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    h->prof = on != 0;
    return TI_OK;
}

int ti_profile_read(ti_handle* h, int kernel, int64_t* n_launches, double* total_ms)
{
    if (!h || kernel < 0 || kernel >= TI_KERNEL_COUNT) return fail(TI_E_ARG, "bad handle / kernel id");
    return guarded([&]() -> int {
        set_device(h);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        double tot = 0; int64_t cnt = 0;
        for (auto& pr : h->ev[kernel]) {
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, pr.first, pr.second));
            tot += ms; ++cnt;
            (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second);
        }
        h->ev[kernel].clear();
        if (n_launches) *n_launches = cnt;
        if (total_ms) *total_ms = tot;
        return TI_OK;
    });
}

int ti_selftest(int device)
{
    return guarded([&]() -> int {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TI_E_HIP, "no HIP device");
        HIP_CHECK(hipSetDevice(device));
        DevBuf<float> d; d.alloc(64 * 16);
        HIP_CHECK(launch_selftest(d.p, nullptr));
        std::vector<float> o(64 * 16);
        HIP_CHECK(hipMemcpy(o.data(), d.p, o.size() * sizeof(float), hipMemcpyDeviceToHost));
        // expected D[i][j] = sum_k A[i][k] B[k][j], A[i][k] = 1 + i + 100k, B[k][j] = 1000 + j - 7k;
        // accumulator register r of lane l holds row (r&3) + 8*(r>>2) + 4*(l>>5), column l&31
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 16; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), j = l & 31;
                double ref = 0;
                for (int k = 0; k < 2; ++k) ref += (1.0 + i + 100.0 * k) * (1000.0 + j - 7.0 * k);
                if (std::fabs(o[l * 16 + r] - ref) > 1e-3 * std::fabs(ref))
                    return fail(TI_E_HIP, "MFMA 32x32x2 lane map differs from the layout the kernels assume (lane " + std::to_string(l) +
                                              ", reg " + std::to_string(r) + ")");
            }
        // the 8-instruction operand split (v_fma_mix lo/hi, half-register writes) against the plain arithmetic, 16.8 M values
        DevBuf<unsigned> cnt; cnt.alloc(2);
        HIP_CHECK(hipMemset(cnt.p, 0, 2 * sizeof(unsigned)));
        HIP_CHECK(launch_split_selftest(cnt.p, nullptr));
        unsigned bad[2] = {0, 0};
        HIP_CHECK(hipMemcpy(bad, cnt.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
        if (bad[0]) return fail(TI_E_HIP, "operand split: " + std::to_string(bad[0]) + " fp16 halves differ from the reference arithmetic (either format)");
        if (bad[1]) return fail(TI_E_HIP, "v_mfma_f32_16x16x32_f16 flushed fp16-subnormal inputs: the one-accumulator operand format needs them kept");
        return TI_OK;
    });
}

}  // extern "C"
