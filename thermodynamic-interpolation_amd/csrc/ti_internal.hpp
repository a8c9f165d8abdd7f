// ti_internal.hpp -- host/device shared declarations of libti_hip.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ti_hip.h"

namespace ti {

// ---- molecule-group edge template -------------------------------------------------------------------------------
// Two templates are built per handle (painn_pack.hip: build_templates): "throughput" (G molecules per group, P = 1: fewest padded
// rows, one wave walks G*E_m rows) and "latency" (G = 1, the destination atoms of a molecule cut into P parts, each part padded
// to whole row blocks and walked by its own wave: P times the waves for small batches).  A kernel's group index counts
// (molecule group, part):  gi = mg * parts + part;  rows / slotnode hold [parts][nblk*16] entries.
// slotnode word: -1 = no such slot, else  atom | molecule-in-group << 8 | SLOT_FIRST_TOUCH: this block is the first one (in the owning
// wave's program order) that holds rows of the atom -- its sums REPLACE the accumulator contents instead of adding to them, so nobody
// has to zero the accumulators between layers.  Set only when every atom of the graph has incoming edges (painn_pack.hip).
constexpr int32_t SLOT_FIRST_TOUCH = 1 << 30;
__host__ __device__ inline int slot_mol(int32_t sn) { return (sn >> 8) & 0x3fffff; }
// The E_m edges of one molecule are sorted by (dst, src); G molecules form a "group" whose G*E_m edge rows are padded
// to NBLK blocks of EDGE_ROWS_PER_BLOCK rows.  One wave owns one group, so every per-atom sum over incoming edges stays inside a wave
// in that wave's program order (deterministic).  Within a block, the distinct (molecule, dst atom) pairs are numbered as "slots";
// a block holds at most EDGE_MAX_SLOTS of them (a fifth destination atom starts the next block, the rest of the block is
// padding), so the per-slot sums of a block fit the four lane rows of a wave (mfma_chain.hpp: r16::QuarterSum).
//   row word : bit0 valid | mol_local<<1 (5b) | src<<6 (5b) | dst<<11 (5b) | etype<<16 (2b) | slot<<18 (6b, 63 = none)
//   slot word: mol_local<<8 | atom     (-1 = unused)
constexpr int ROW_VALID = 1;
constexpr int EDGE_ROWS_PER_BLOCK = 16;     // painn_edge_kernel walks a group in 16-row blocks (16x16x4 MFMA)
constexpr int EDGE_MAX_SLOTS = 4;
__host__ __device__ inline int row_mol(uint32_t w) { return (w >> 1) & 31; }
__host__ __device__ inline int row_src(uint32_t w) { return (w >> 6) & 31; }
__host__ __device__ inline int row_dst(uint32_t w) { return (w >> 11) & 31; }
__host__ __device__ inline int row_type(uint32_t w) { return (w >> 16) & 3; }
__host__ __device__ inline int row_slot(uint32_t w) { return (w >> 18) & 63; }

// ---- pair-major template (painn_pair_kernel.hpp; painn_pack.hip: build_pair_template).  The filter branch w(enc(|r_ij|)) of SE3Message
// (cpainn.py:283-289) depends on the edge length only, so the edges i->j and j->i share it bit for bit.  A row block holds 16 atom PAIRS
// laid out as a 4 x 4 tile: row 4a + b = pair (I[a], J[b]) of up to four "I" atoms and four "J" atoms (slots carry molecule-in-group and
// atom; rows of pairs that do not exist are invalid).  Direction A is the edge I[a] -> J[b] (src I, dst J), direction B the edge
// J[b] -> I[a].  The per-atom sums need no masks: direction B's destination is the same for the four rows a lane holds (in-lane adds),
// direction A's is the same across the four lane rows (two lane-swap levels).  A packed template (pair_template.hpp) ends with GENERAL
// blocks: 16 unrelated pairs named by their row words alone, slot words -1, no first touch; every row adds to its own two atoms.
//   row word : bit0 valid | molI<<1 (3b) | atomI<<4 (5b) | molJ<<9 (3b) | atomJ<<12 (5b) | etype<<17 (2b)     (empty slots: a safe atom)
//   slot word: slotnode[blk*16 + k], k = 0..3 the I slots, k = 4..7 the J slots: -1, or atom | mol<<8
// Per-atom sums: the wave that owns the group adds the sums of slot k of block b to the atom's accumulator rows with fire-and-forget
// atomics, in walk order (blocks ascending, inside a block the J slots before the I slots); the first slot that holds an atom in that
// order carries SLOT_FIRST_TOUCH and replaces the stale contents (pair_template.hpp).
// e rows: [group][block][direction][16][F]; the parked encoding / edge_dir (direction A's) once per pair: [group][block][16].
constexpr int PAIR_MAX_G = 8;
__host__ __device__ inline int prow_molI(uint32_t w) { return (w >> 1) & 7; }
__host__ __device__ inline int prow_atomI(uint32_t w) { return (w >> 4) & 31; }
__host__ __device__ inline int prow_molJ(uint32_t w) { return (w >> 9) & 7; }
__host__ __device__ inline int prow_atomJ(uint32_t w) { return (w >> 12) & 31; }
__host__ __device__ inline int prow_type(uint32_t w) { return (w >> 17) & 3; }

struct MlpVec {           // natural-order per-feature vectors of one reference MLP block (device pointers)
    const float *b0, *g0, *be0, *b1, *g1, *be1, *b2;
};

struct EdgeParams {
    const float4* stream; int nch;         // packed weight chunks of this layer's message block
    const float* vecs;                      // [21][F] bias/gamma/beta of the w and phi MLPs (painn_kernels.hip: struct EV)
    const float* edge_emb;                  // [4][F]  (first layer: e = edge_emb[type])
    const uint32_t* rows; const int32_t* slotnode; const int32_t* nslots;
    int nblk, G, parts, A;                  // parts per group (see above); n_groups counts parts
    int max_slots;                          // most destination atoms any row block of the template holds (<= 4)
    int n_tile;                             // pair launches: blocks [0, n_tile) are tiles, [n_tile, nblk) general (== nblk: tiles only)
    int row_stride;                         // the general pair launch: row words per group in `rows` (0: the template's, shared by all groups)
    long long B, n_groups;
    float length_scale;
    const float* x;                         // [B*A][3]
    const float* P;                         // [B*A][F]   s @ W0[:, :F]^T + b0
    const float* v;                         // [B*A][3][F]
    float* dsacc;                           // [B*A][F]   += sum ds   (added to s by the update kernel)
    float* dvacc;                           // [B*A][3][F] += sum (sed*dir + gates*v[src])
    float* cacc;                            // [B*A][3][F] += sum cg*dir   (crossed with v[dst] in the update kernel; not written by a
                                            //   pair launch that folds the cross term, pair_folds_cross)
    float* e;                               // [n_groups*nblk*16][F]
    float* enc;                             // [n_groups*nblk][operand registers][64] parked encoding operand of every row block (layer 0 writes, the others read)
    float wscale[6];                        // TI_PREC_F16X2: powers of two the host scaled w.W0, w.W1, phi.W0(e), phi.W1, phi.W2, w.W2 by (else 1)
    float* geo;                             // [n_groups*nblk*16][4] parked edge_dir
    unsigned long long* stamps;             // diagnostic builds (-DTI_STAMPS) only: s_memtime / s_memrealtime stamps, a buffer of their own; else NULL
    // layer-0 phi table (the TABLE builds of the pair kernel, painn_pair_kernel.hpp; NULL / 0 for every other launch): `stream` then
    // holds the w chunks alone (painn_pack.hip: st_phi0_w)
    const float* phi0_tab;                  // [class][A][PHI0_TYPES][3][F]: ds | scale_edge_dir | de slices of the phi branch, bias included
    const uint8_t* cls;                     // [B] class of every molecule (painn_phi0_kernels.hip)
    int wpad;                               // the w-only stream ends with a pad chunk (odd count), swallowed once per row block
    // merged tails (painn_pair_general_tails_kernel; pair_template.hpp: pair_template_tails; 0 for every other launch): a wave owns
    // tail_S groups, whose last general blocks hold tail_r = 16 / tail_S valid rows each and are walked as one block
    int tail_S, tail_r;
};

// ---- layer-0 phi table (painn_phi0_kernels.hip; include/ti_hip.h TI_PHI0_MAX_CLASSES)
constexpr int PHI0_TYPES = 4;               // edge types a row word can name (2 bits): the table holds them all
static_assert(TI_PHI0_MAX_CLASSES <= 16, "the pair kernel packs the class ids of a group's <= 8 molecules into one 32-bit word");
// class state on the device: [0 .. CAP) the representative molecule of each class (-1: none yet), [CAP] 1 = more classes than the cap
constexpr int PHI0_STATE_WORDS = TI_PHI0_MAX_CLASSES + 1;
struct Phi0ClassParams {
    const uint32_t* cond; int words;        // [B][words] the cond rows of a molecule as bit patterns (words = A * ncond, may be 0)
    long long B;
    int32_t* state;                         // [PHI0_STATE_WORDS], filled with -1 before the launch
    uint8_t* cls;                           // [B]
};
struct Phi0TableParams {
    const float4* stream; int nch;          // the phi chunks of layer 0 alone (painn_pack.hip: st_phi0_tab)
    const float* vecs; const float* edge_emb; float wscale[6];      // as EdgeParams (one-accumulator format)
    const float* P;                         // [B*A][F] of this evaluation's embed launch; state == NULL: the compact P_cls [n_cls*A][F]
    const int32_t* state;                   // class representatives; NULL: P holds the classes' rows themselves (embed per class)
    int n_cls, A;
    float* tab;
};
hipError_t launch_phi0_classes(const Phi0ClassParams& p, hipStream_t st);
hipError_t launch_phi0_table(int NB, bool last, const Phi0TableParams& p, hipStream_t st);
hipError_t configure_phi0_kernels(int NB);
// the table builds of the pair kernel: the split path, unmasked, both wave counts
__host__ __device__ constexpr bool pair_table_build_exists(int NB, int PREC, bool MASK) { return PREC == TI_PREC_F16X2 && !MASK && (NB == 1 || NB == 2 || NB == 4); }

struct EmbedParams {
    const float4* stream; int nch;
    MlpVec mlp; const float* pb0;           // pb0 = phi[0].b0
    const float* atom_emb; const int32_t* atom_ids; const float* cond;
    int ncond, A; long long N;
    float t, temp_length, time_length, temp_mean, temp_range;
    const float* tv;                        // non-NULL: per-molecule times [B] (node nd reads tv[nd / A]) instead of t
    float* s; float* P;
    const int32_t* rep;                     // REP builds: class representatives; node n = (class, atom) reads molecule rep[n / A]'s cond rows, s / P are [n_cls*A][F]
};

struct UpdateParams {
    const float4* stream; int nch;
    const float* vecs;                      // [10][F] (painn_kernels.hip: struct UV)
    long long N;
    float *s, *v, *dsacc, *dvacc, *cacc, *P;
    int first_layer;                        // v and cacc are zero by definition (nothing has written them yet): not read
    int zero_acc;                           // reset the accumulators after use (0 when the edge kernels overwrite on first touch)
    // SCLS builds (layer 0 after an embed per class): the incoming s is s_cls[cls[node / A]][node % A] instead of s[node]
    const float* s_cls; const uint8_t* cls; int A;
};

struct ReadoutParams {
    const float4* stream; int nch;
    MlpVec mlp; const float* w2_gate; float b2_gate; const float* Vr;
    long long N;
    const float *s, *v; float* out;
};

// launchers (painn_kernels.hip).  F = 32*NB; return hipError_t of the launch.
// prec = TI_PREC_* of include/ti_hip.h; with TI_PREC_F16 the state tensors s, P, v, e behind the float* fields are fp16
// p.rep non-NULL: the per-class build (f16x2, scalar t), p.N = n_cls * A rows
hipError_t launch_embed(int NB, int nseg, int prec, const EmbedParams& p, hipStream_t st);
// masked: the masked twins of the message kernels (per-molecule edge sets, ti_painn_set_edge_mask); p.rows then holds row words per
// (group, part) instead of the template's (painn_pack.hip: masked_rows)
hipError_t launch_edge(int NB, bool first, bool last, int prec, const EdgeParams& p, hipStream_t st, bool masked = false);
// The message kernels (directed and pair-major) run TI_PREC_F16X2 on the one-accumulator split format (mfma_chain.hpp: Opnd1), at every
// width; painn_pack.hip packs their streams and vector blocks to match.
__host__ __device__ constexpr bool edge_one_chain(int prec) { return prec == TI_PREC_F16X2; }
// pair-major message kernel (painn_pair_kernel.hpp): same EdgeParams, rows / slotnode of the pair template, same weight stream
// table: layer 0 on the phi table (p.phi0_tab / p.cls / p.wpad set, p.stream the w-only stream; first must hold, pair_table_build_exists)
// Two launches when the template has general blocks (p.n_tile < p.nblk): the tile builds over [0, n_tile), then the general builds.
// seeded (a seeded template, pair_template.hpp; split path, unmasked, one species): the seeded general builds FIRST -- plain stores,
// every atom's first contribution of the layer -- then the seeded tile builds, which only add.
hipError_t launch_pair(int NB, bool first, bool last, int prec, const EdgeParams& p, hipStream_t st, bool masked = false, bool table = false,
                       bool seeded = false);
// builds of the pair kernel (painn_pair_kernel.hpp): F <= 128; f32 on 4 waves, split fp16 on 4 and on 8
__host__ __device__ constexpr bool pair_build_exists(int NB, int WAVES, int PREC)
{
    return (NB == 1 || NB == 2 || NB == 4) && (PREC == TI_PREC_F32 ? WAVES == 4 : PREC == TI_PREC_F16X2 && (WAVES == 4 || WAVES == 8));
}
// the builds for the general blocks of a packed pair template (pair_template.hpp): the split path.  The f32 builds, short of registers
// as they are, spill with eight destination atoms per lane (36 - 56 registers at F = 128): f32 handles keep the tile-only template.
__host__ __device__ constexpr bool pair_general_build_exists(int PREC) { return PREC == TI_PREC_F16X2; }
// the pair kernel at this precision adds (sum cg*dir) x v[dst] to dvacc itself, per row block and slot (painn_pair_kernel_body.inc,
// FOLD), and leaves cacc alone: the update kernel after it must be the folded one (launch_update(.., folded = true)).  The split path
// only: it holds v[dst] of both directions in registers.  Its 4- and 8-wave builds both fold, so that a slice of groups evaluated
// alone stays bit for bit what it is in a larger batch.  The f32 path keeps the cross-gate sums in cacc.
__host__ __device__ constexpr bool pair_folds_cross(int prec) { return prec == TI_PREC_F16X2; }
// folded: the message launch before it already added the cross term to dvacc (pair_folds_cross); cacc is then neither read nor reset
// keep: the twin build that keeps v_eff in registers between its phases instead of parking it in dvacc (painn_update_keep.hip; the same
// results bit for bit); update_keep_components: how many of the three components that build keeps, 0 where there is no such build
hipError_t launch_update(int NB, bool has_next, int prec, const UpdateParams& p, hipStream_t st, bool folded = false, bool keep = false);
int update_keep_components(int NB, int prec);
hipError_t configure_update_keep(int NB);                                        // painn_update_keep.hip
hipError_t launch_update_keep(int NB, bool has_next, int prec, const UpdateParams& p, hipStream_t st, bool folded);
hipError_t launch_readout(int NB, int prec, const ReadoutParams& p, hipStream_t st);
hipError_t configure_painn_kernels(int NB);     // dynamic-LDS attributes
// What the one-width translation units of the message kernels export (painn_{edge,pair}[_mask]_nb*.hip, one unit per width so that they
// compile in parallel): defined in painn_edge_kernel.hpp / painn_pair_kernel.hpp, explicitly instantiated once per (NB, MASK) in its
// unit, reached from launch_edge / launch_pair / configure_painn_kernels (painn_kernels.hip).  No pair unit exists for NB = 8.
template <int NB, bool MASK> hipError_t launch_edge_unit(bool first, bool last, int prec, const EdgeParams& p, hipStream_t st);
template <int NB, bool MASK> hipError_t configure_edge_unit();
// (GENERAL: the builds that walk a packed template's general blocks, units painn_pair_gen_nb*.hip; MASK is false for them.
// SEEDED: the seeded twins of the unmasked tile and general builds, units painn_pair_seed_nb*.hip)
template <int NB, bool MASK, bool GENERAL, bool SEEDED = false> hipError_t launch_pair_unit(bool first, bool last, int prec, const EdgeParams& p, hipStream_t st, bool table);
template <int NB, bool MASK, bool GENERAL, bool SEEDED = false> hipError_t configure_pair_unit();
// (the merged-tails builds of the seeded general launch, units painn_pair_tails_nb*.hip)
template <int NB> hipError_t launch_pair_tails_unit(bool first, bool last, const EdgeParams& p, hipStream_t st, bool table);
template <int NB> hipError_t configure_pair_tails_unit();

// ---- forward-mode derivative of the drift (painn_jvp_kernels.hip; virtual-molecule layout described there).
// D = 3A and xdot == NULL: unit seeds (direction d -> atom d/3, component d%3); otherwise D explicit directions xdot [B][D][A][3]
// (D = 1: ti_painn_drift_jvp; D = k: the Hutchinson probes).
// Tangent arrays are laid out like their primal twins over ceil(B/G)*D*G virtual molecules; primal arrays are read only.
struct JvpFilterParams {                    // primal pass of one layer's message block (painn_jvp_filter_kernel)
    const float4* stream; int nch; const float* vecs; const float* edge_emb;      // the primal edge stream / vector block
    const uint32_t* rows;
    int nblk, G, parts, A, first, last;
    long long B, n_groups;                  // molecules, primal groups (incl. parts)
    float length_scale;
    const float *x, *P, *e;
    float4* wq;                             // [n_groups*nblk][5][NB][6][64] float4: phi_o, w_o, d w_o / d|r|
    float4* st;                             // [n_groups*nblk][4][NBK][64]   float4: LayerNorm statistics of phi
};
struct JvpEdgeParams {
    const float4* stream; int nch, pad; const float* vecs; const float* edge_emb;
    const uint32_t* rows; const int32_t* slotnode;
    int nblk, G, parts, A, D, first, last;
    long long B, n_groups;                  // molecules, VIRTUAL groups (= molecule groups * D * P)
    const float *x, *xdot;
    const float *P, *v, *e;                 // primal state entering this layer's message block
    const float4 *wq, *st;                  // primal pass output of this layer
    const float *tP, *tv;                   // tangents of P and v
    float *te, *tdsacc, *tdvacc, *tcacc;    // tangent of e (updated in place), tangent accumulators (+=)
};
struct JvpNodeParams {                      // primal node pass of one layer's update block (painn_jvp_node_kernel)
    const float4* stream; int nch; const float* vecs;          // the tangent update stream (V and U once per component)
    long long N;                            // primal nodes
    const float *s, *v, *dsacc, *dvacc, *cacc;
    float4* ns;                             // [ceil(N/16)][13][NBK][64] float4
};
struct JvpUpdateParams {
    const float4* stream; int nch; const float* vecs;
    long long N, B; int A, D, G, has_next;  // N virtual nodes
    const float *v, *cacc;                  // primal, as the primal edge kernel left them
    const float4* ns;                       // primal node pass output of this layer
    float *ts, *tv, *tdsacc, *tdvacc, *tcacc, *tP;
    int zero_acc;                           // reset the tangent accumulators after use (0 with first-touch slot tables)
};
struct JvpReadoutParams {
    const float4* stream; int nch; const float* vecs; float b2_gate;      // vecs: b0 g0 be0 b1 g1 be1 w2_gate Vr (x F)
    long long N, B; int A, D, G;
    const float *s, *v, *ts, *tv;
    float* tout;                            // [virtual nodes][3]
};
// masked: p.rows holds row words per (group, part) with each molecule's own edge types (ti_painn_set_molecules with pair_type)
hipError_t launch_jvp_filter(int NB, bool split, const JvpFilterParams& p, hipStream_t st, bool masked = false);
hipError_t launch_jvp_edge(int NB, bool split, const JvpEdgeParams& p, hipStream_t st, bool masked = false);
hipError_t launch_jvp_node(int NB, bool split, const JvpNodeParams& p, hipStream_t st);
hipError_t launch_jvp_update(int NB, bool split, const JvpUpdateParams& p, hipStream_t st);
hipError_t launch_jvp_readout(int NB, bool split, const JvpReadoutParams& p, hipStream_t st);
hipError_t launch_div_reduce(const float* tout, long long B, int D, int G, float* div, hipStream_t st);
// est[b] = (1/k) sum_{p,i} eps[b][p][i] tout[virtual molecule (b, p)][i], eps [B][k][3A]; one wave per molecule, fixed order
hipError_t launch_hutch_reduce(const float* tout, const float* eps, long long B, int k, int A, int G, float* est, hipStream_t st);
hipError_t configure_painn_jvp_kernels(int NB);

// ---- adw (adw_kernels.hip).  One kernel evaluates  Linear(3->H), SiLU, [Linear(H->H), SiLU] x n_hidden, Linear(H->1)
// on rows (a0, a1, a2):  a0 = x[r];  a1 = in1 ? in1[r] : t;  a2 = idx ? emb[idx[r]] : emb ? emb[r] : t.
struct AdwParams {
    const float4* stream; int nch;          // hidden layers, 32-output chunks (16-row format), layer-major
    const float* vecs;                      // w_in [H][3] | b_in [H] | b_hidden [n_hidden][H] | w_out [H]
    float b_out;
    int n_hidden; long long B;
    const float* x; const float* in1; const float* emb; const int32_t* idx;
    float t;
    float* out;
    float* out_div;                         // non-NULL: also d out / d a0 (forward-mode tangent)
    int dim;                                // 0 / 1: the layout above.  2..16: the d-dimensional net (adw_mlp_nd_kernel): x and out
                                            // [B][dim], vecs w_in [H][Kpad] | b_in | b_hidden | w_out [dim][H] | b_out [dim], and
                                            // out_div = sum_i d out_i / d x_i
};
hipError_t launch_adw(int NB, bool split, const AdwParams& p, hipStream_t st);
hipError_t configure_adw_kernels(int NB, int max_hidden, int dim);

// ---- fused adw rollout (adw_fused_kernels.hip; include/ti_hip.h ti_adw_rollout_fused): one launch runs all n_step - 1 steps of a 1-D
// handle.  The host fills the per-step scalars with the fp32 expressions of rollout_common (rollout.hpp); the kernel computes none.
enum { ADW_FUSED_EULER = 0, ADW_FUSED_HEUN = 1, ADW_FUSED_EM = 2 };       // EM: Euler plus the noise term (eps > 0)
struct AdwFusedStep {                       // step k: t_grid[k] -> t_grid[k + 1]
    float t, t_next;                        // t_grid[k], t_grid[k + 1]
    float dt, hdt;                          // t_grid[k + 1] - t_grid[k];  0.5f * dt
    float ndt, nhdt;                        // -dt * div_scale;  -0.5f * dt * div_scale   (dlogp state)
    float sigma;                            // sqrt(2 eps |dt|)
    float pad;
};
struct AdwFusedParams {
    const float4* stream; int nch;          // `net`: as AdwParams
    const float* vecs;
    float b_out;
    int n_hidden; long long B;
    float* x;                               // [B] in: x0, out: the end state
    const int32_t* idx;                     // [B] row -> deduplicated (beta0, beta1) pair
    const float* emb; long long U;          // [n_step][U] beta embedding at every grid point: emb[k * U + idx[row]]
    const AdwFusedStep* steps;              // [n_step - 1]
    int n_step, save_every, scheme;         // scheme: ADW_FUSED_*
    uint64_t seed; long long traj0; int step0;      // EM: ti_normal(seed, traj0 + row, step0 + k, 0)
    float* out_path;                        // [rows][B]
    float* out_dlogp; float out_scale;      // non-NULL: [rows][B] = dlogp * out_scale (selects the tangent instantiation)
};
hipError_t launch_adw_fused(int NB, bool split, const AdwFusedParams& p, hipStream_t st);
hipError_t configure_adw_fused_kernels(int NB, int max_hidden);

// ---- integrator kernels (integrate_kernels.hip)
hipError_t launch_axpy(float* y, const float* x, float a, const float* b, long long n, hipStream_t st);          // y = x + a*b
hipError_t launch_heun(float* x, float hdt, const float* b1, const float* b2, long long n, hipStream_t st);      // x += hdt*(b1+b2)
hipError_t launch_noise(float* x, float sigma, uint64_t seed, long long traj0, int step, long long B, int comps_per_traj,
                        int atoms_for_com /*0 = no COM removal*/, hipStream_t st);
// eps [B][k][comps] = +1 / -1 by the sign of the noise normal (seed, traj0 + b, step = p, component i); 0 -> +1
hipError_t launch_probes(float* eps, uint64_t seed, long long traj0, long long B, int k, int comps, hipStream_t st);
hipError_t launch_scale(float* y, const float* x, float a, long long n, hipStream_t st);                            // y = a*x
hipError_t launch_selftest(float* out /*[64*16]*/, hipStream_t st);
hipError_t launch_split_selftest(unsigned* out /*[2], zeroed: differing halves, subnormal-product mismatches*/, hipStream_t st);
hipError_t launch_nan_check(const float* x, long long n, int* flag, hipStream_t st);
// ---- mixed-species batches (ti_painn_set_molecules): arrays of [mols][A][comps] floats, molecule i has n_atoms[i / rep] real atoms
// dst = src on real atoms; on pad atoms 0, or with park_coords (comps = 3) the parking place x[mol][0] + (100 (a - n + 1), 0, 0)
hipError_t launch_park_pads(float* dst, const float* src, const int32_t* n_atoms, long long mols, int rep, int A, int comps, int park_coords,
                            hipStream_t st);
hipError_t launch_zero_pads(float* y, const int32_t* n_atoms, long long mols, int rep, int A, int comps, hipStream_t st);      // y = +0 on pads
hipError_t launch_copy_pads(float* dst, const float* src, const int32_t* n_atoms, long long mols, int A, int comps, hipStream_t st);   // dst = src on pads
// launch_noise over the 3 n_atoms[b] real components of each molecule ([B][A][3]); com: centre of mass over the real atoms
hipError_t launch_noise_ragged(float* x, float sigma, uint64_t seed, long long traj0, int step, long long B, int A, int com,
                               const int32_t* n_atoms, hipStream_t st);
// launch_div_reduce (D = 3A unit seeds) summing the 3 n_atoms[b] real directions of each molecule only
hipError_t launch_div_reduce_ragged(const float* tout, long long B, int D, int G, const int32_t* n_atoms, float* div, hipStream_t st);

// ---- Runge-Kutta pieces (ode_kernels.hip)
struct RkComb { const float* k[7]; float c[7]; int nk; };     // sum_j c[j] * k[j][i], j < nk
constexpr int RED_PARTIALS = 1024;                             // size of the `partial` scratch (doubles) of the reductions below
hipError_t launch_rk_combo(float* y, const float* y0, const RkComb& c, long long n, hipStream_t st);               // y = y0 + comb
// *out = sum_i (comb_i / (atol + rtol max(|y0_i|, |y1_i|)))^2, fixed summation order
hipError_t launch_rk_ratio_sumsq(double* out, double* partial, const float* y0, const float* y1, const RkComb& c, float rtol, float atol,
                                 long long n, hipStream_t st);
// *out = sum_i ((a_i - b_i) / (atol + rtol |y0_i|))^2   (b may be NULL)
hipError_t launch_scaled_sumsq(double* out, double* partial, const float* a, const float* b, const float* y0, float rtol, float atol,
                               long long n, hipStream_t st);
// ragged twins (ode_ragged_kernels.hip, ti_painn_set_molecules): the state is [B][m] with m = 3A floats per molecule of which the first
// 3 n_atoms[b] are real; pad entries are skipped in the same summation order (the caller divides by the real count)
hipError_t launch_rk_ratio_sumsq_ragged(double* out, double* partial, const float* y0, const float* y1, const RkComb& c, float rtol, float atol,
                                        long long n, const int32_t* n_atoms, int m, hipStream_t st);
hipError_t launch_scaled_sumsq_ragged(double* out, double* partial, const float* a, const float* b, const float* y0, float rtol, float atol,
                                      long long n, const int32_t* n_atoms, int m, hipStream_t st);
hipError_t launch_interp_fit(float* coef /*[5][n]*/, const float* y0, const float* y1, const float* f0, const float* f1, const RkComb& mid,
                             float dt, long long n, hipStream_t st);
hipError_t launch_interp_eval(float* out, const float* coef, float x, long long n, hipStream_t st);

// ---- per-trajectory dopri5 (ode_kernels.hip; driver: rollout.hpp rollout_rk_traj).  Every trajectory b runs the shared algorithm
// on its own: segment s holds m_s floats per trajectory (segment 0: x, 3A or 1; segment 1: its dlogp entry, m = 1), laid out
// trajectory-major.  Controller state is fp64 in the integration variable s = sign * t.  A trajectory whose interval has passed the
// last grid time is frozen: its state, k and path rows are never written again (it still rides along in the batched drift launches).
struct TrajCtl {
    double t0, t1, dt;              // interval [t0, t1] of the last accepted step (dense output), next step size
    double h0, d1;                  // initial-step scratch (_select_initial_step)
    int next;                       // next grid index to emit; == n_grid: finished
    int rows;                       // path rows written so far
    int accepted, rejected;
};
struct TrajSeg {
    float *y, *ytmp, *ynew, *coef;  // coef: [5][B*m]
    float* k[7];
    float* out;                     // path rows [rows][B*m] (device: the caller's buffer or a staging copy)
    long long m;
    float out_scale;                // rows are written * out_scale (the dlogp convention; 1 for x)
};
enum { TRAJ_ST_ACTIVE = 0, TRAJ_ST_MISSING = 1, TRAJ_ST_UNDERFLOW = 2, TRAJ_ST_NAN = 3, TRAJ_ST_LIMIT = 4, TRAJ_ST_N = 8 };
struct TrajRkParams {
    TrajSeg seg[2]; int nseg;
    long long B;
    TrajCtl* ctl;
    float* tv;                      // [B] fp32 drift time of each trajectory for the next evaluation (original t, sign applied)
    int* status;                    // [TRAJ_ST_N]: active count, most rows any trajectory still owes (reset per attempt); the first
                                    // trajectory that underflowed / got a NaN ratio / passed the attempt limit (INT_MAX: none)
    const double* grid;             // [n_grid] sign * t_grid
    int n_grid, save_every, total_rows;
    double sign, t_first;
    float rtol, atol;
    long long max_attempts;
};
// phase 0: d0, d1, h0 from y and k[0], ytmp = y + h0 k[0], tv = t_first + h0;  phase 1: d2 from k[1], dt, controller reset
hipError_t launch_traj_init(const TrajRkParams& p, int phase, hipStream_t st);
// stage input y + sum_{j<nk} (c_j dt_b) k_j into ytmp (to_ynew = 0) or ynew, and tv[b] = t_b + alpha dt_b (alpha_one: one ulp
// below t_b + dt_b); frozen trajectories copy y.  stage 0 also checks step underflow and the attempt limit.
hipError_t launch_traj_stage(const TrajRkParams& p, const float* c, int nk, float alpha, int alpha_one, int to_ynew, int stage0,
                             hipStream_t st);
// error ratio, accept / reject, dense-output fit, FSAL copy, step factor, emission of the grid rows the accepted step crossed
hipError_t launch_traj_advance(const TrajRkParams& p, const float* c_error /*[7]*/, const float* c_mid /*[7]*/, hipStream_t st);
// ragged twins of the three (ode_ragged_kernels.hip): segment 0's norms over the first 3 n_atoms[b] of its m entries, pad entries kept
hipError_t launch_traj_init_ragged(const TrajRkParams& p, int phase, const int32_t* n_atoms, hipStream_t st);
hipError_t launch_traj_stage_ragged(const TrajRkParams& p, const float* c, int nk, float alpha, int alpha_one, int to_ynew, int stage0,
                                    const int32_t* n_atoms, hipStream_t st);
hipError_t launch_traj_advance_ragged(const TrajRkParams& p, const float* c_error, const float* c_mid, const int32_t* n_atoms, hipStream_t st);

// ---- observables (obs_kernels.hip; include/ti_hip.h ti_obs_*)
struct ObsCvParams {
    const float* x;                         // [B][m] floats: m = 3A (molecules) or the adw dimension
    long long B; int A, m, K;
    const int32_t* desc;                    // [K][5] (kind, i, j, k, l), validated on the host
    const float* ref;                       // [A][3] RMSD reference frame (NULL without an RMSD descriptor)
    const int32_t* sel;                     // [A] 0 / 1 RMSD selection, NULL: every atom
    const int32_t* n_atoms;                 // [B] real atoms per molecule (mixed species), NULL: A
    float* cv;                              // [B][K]
};
// Launch shape of the batch-wide sums: obs_blocks(B) blocks of 256 threads walk the B values grid-stride.  Few blocks on purpose:
// the per-bin wave sums make a histogram cost O(bins present) shuffles per 64 values whatever the grid, the second pass stays one
// short loop per column, and at the product's batch sizes (<= 1e5) these calls are bound by their launches, not by their width.
constexpr int OBS_MAX_BLOCKS = 8;
int obs_blocks(long long B);
hipError_t launch_obs_cv(const ObsCvParams& p, hipStream_t st);
// out[0] = largest finite logw (-inf: none), out[1] = smallest index of a non-finite entry as a double (+inf: none); partial: [OBS_MAX_BLOCKS][2]
hipError_t launch_obs_logw_max(double* out, double* partial, const float* logw, long long B, hipStream_t st);
// out[0] = sum w, out[1] = sum w^2, w = exp(logw - *mx)
hipError_t launch_obs_logw_sums(double* out, double* partial, const float* logw, const double* mx, long long B, hipStream_t st);
// w[i] = exp(logw[i] - norm[0]) / norm[1]
hipError_t launch_obs_weights(float* w, const float* logw, const double* norm, long long B, hipStream_t st);
// out [n_bins + 3]: the histogram of values[i * stride] on [lo, hi) weighted by exp(logw - norm[0]) / norm[1] (logw == NULL: 1 / B),
// then the weights below lo, at or above hi, and of non-finite values; partial: [OBS_MAX_BLOCKS][n_bins + 3]
hipError_t launch_obs_whist(double* out, double* partial, const float* values, long long stride, const float* logw, const double* norm, long long B,
                            int n_bins, double lo, double hi, hipStream_t st);

// ---- force-field energies (obs_ff_kernels.hip; include/ti_hip.h ti_obs_ff_*, ti_obs_ti_logw)
// A term's atoms and flags in one word: i | j << 5 | k << 10 | l << 15 | n << 20 (torsion periodicity) | FF_LIVE (pair rows that are
// evaluated).  The words of the four tables follow each other (bonds, angles, torsions, pairs), as do their parameters: bonds
// [nb][2] (r0, k), angles [na][2] (theta0, k), torsions [nt][2] (phase, k), pairs [np][3] (qq, sigma, eps).
constexpr int FF_WAVES = 4;                 // molecules in flight per 256-thread workgroup, one wave each
constexpr int FF_MAX_ATOMS = 25;            // TI_FF_MAX_PAIRS = 25 * 24 / 2
constexpr int32_t FF_LIVE = 1 << 24;
__host__ __device__ inline int ff_atom(int32_t w, int slot) { return (w >> (5 * slot)) & 31; }
__host__ __device__ inline int ff_period(int32_t w) { return (w >> 20) & 7; }
struct FfParams {
    const float* x;                         // [B][A][3]
    const float* T;                         // [B] kelvin, NULL: energies in kJ/mol
    long long B; int A;
    double to_nm, coulomb;
    int nb, na, nt, np;                     // table lengths, within the TI_FF_MAX_* caps (checked on the host)
    const int32_t* idx;                     // [nb + na + nt + np] term words
    const double* par;                      // [2 nb + 2 na + 2 nt + 3 np]
    double* e;                              // [B]
    double* terms;                          // [B][4] or NULL
};
hipError_t launch_obs_ff_energy(const FfParams& p, hipStream_t st);
// out[0] = the smallest index b with T[b] <= 0 or not finite, as a double (+inf: none)
hipError_t launch_obs_ff_bad_temperature(double* out, const float* T, long long B, hipStream_t st);
// logw[b] = (float)-((u1[b] - u0[b]) + neg_dlogp[b]) in fp64; u0 / neg_dlogp NULL: 0
hipError_t launch_obs_ti_logw(float* logw, const double* u0, const double* u1, const float* neg_dlogp, long long B, hipStream_t st);

// ---- Boltzmann-generator log-weights (obs_bg_kernels.hip; include/ti_hip.h ti_obs_bg_logw)
struct BgParams {
    const float* z;                         // [B][m] prior samples
    long long B; int m;
    const double* u1;                       // [B] reduced energy of the generated state, NULL: 0
    const float *nd_bg, *nd_ti;             // [B] each, NULL: 0
    double* logpz;                          // [B] or NULL: -(0.5 sum z^2) - (m HALF_LOG_2PI)
    float* logw;                            // [B] or NULL: (float)-(((u1 + logpz) + nd_bg) + nd_ti)
};
hipError_t launch_obs_bg_logw(const BgParams& p, hipStream_t st);
// the ESS of the unrounded fp64 log-weights of the kept molecules (include/ti_hip.h ti_obs_bg_ess)
struct BgEssParams {
    const double *logpz, *u1;               // [B]; u1 NULL: 0
    const float *nd_bg, *nd_ti;             // [B] each, NULL: 0
    const uint8_t* keep;                    // [B] or NULL: all
    long long B;
    double* out;                            // (ess, kept count, first index of a non-finite kept log-weight or +inf)
};
hipError_t launch_obs_bg_ess(const BgEssParams& p, hipStream_t st);

// ---- force-field forces and Langevin dynamics (obs_ff_md_kernels.hip, ff_device.hpp; include/ti_hip.h ti_obs_ff_forces,
// ti_obs_ff_langevin).  The tables are those of FfParams plus the incidence list of the bonded terms (ff_device.hpp).
struct FfTablesDev {
    int A, nb, na, nt, np;
    double coulomb;
    const int32_t* idx; const double* par;  // as in FfParams
    const int32_t* inc; int inc_words;      // the packed incidence list
};
struct FfForceParams {
    FfTablesDev t;
    const float* x; const float* T;         // [B][A][3]; [B] kelvin or NULL
    long long B; double to_nm;
    double* f; double* e;                   // [B][A][3]; [B] or NULL
};
hipError_t launch_obs_ff_forces(const FfForceParams& p, hipStream_t st);
struct MdParams {
    FfTablesDev t;
    double *pos, *vel;                      // [B][A][3] fp64 nm, nm/ps: the state, read at the start and written at the end of a launch
    const float* T; const long long* ids;   // [B] kelvin; [B] or NULL (replica b: traj_offset + b)
    const double* mass;                     // [A] amu
    long long B, traj_offset;
    double dt, a, to_nm;                    // a = exp(-friction dt) (1: no thermostat, no draw)
    long long n_steps, steps_before, stride, n_frames;      // this launch's steps; the call's steps before it; frames of the call
    long long step0;                        // global index of this launch's first step
    unsigned long long seed;
    int draw, launch;                       // draw: velocities drawn before the first step (first launch only)
    float* frames; double *epot, *ekin;     // [B][n_frames][A][3]; [B][n_frames]; each may be NULL
    int* flag;                              // [B]: 0, or 1 + the launch in which the replica's state turned non-finite
    const double* bad_T;                    // launch_obs_ff_bad_temperature's output: below B, the launch does nothing
};
hipError_t launch_obs_ff_langevin(const MdParams& p, hipStream_t st);

// ---- replica exchange between Langevin launches (obs_ff_remd_kernels.hip; include/ti_hip.h ti_obs_ff_remd).  Row l K + k is rung k
// of ladder l; one launch is one attempt: it evaluates the energies of the rows of its pairs, decides and exchanges them in place.
struct RemdParams {
    FfTablesDev t;
    double *pos, *vel;                      // [B][A][3]: the working state of the Langevin launches
    const float* T;                         // [B] kelvin
    const long long* ladder_ids;            // [B / K] or NULL (ladder l: l)
    const double* mass; double dt;          // [A] amu and the step: the half kick (dt / 2) f / m between stored and on-step velocities
    long long B; int K;
    long long attempt;                      // n: pairs (k, k + 1) with k % 2 == n % 2; its low 32 bits are the third counter word
    unsigned long long seed;
    int32_t* walker;                        // [B]: the working labels, exchanged with the state
    int32_t* out_walker;                    // [B]: the labels after this attempt, or NULL
    long long* counts;                      // [B / K][K - 1][2]: attempts and acceptances of the call so far, or NULL
    const int* flag;                        // MdParams::flag: a stopped replica takes part in no pair
    const double* bad_T;                    // below B (a refused temperature or walker label): the launch does nothing
};
hipError_t launch_obs_ff_remd(const RemdParams& p, hipStream_t st);
// work[b] = in ? in[b] : b % K.  A label outside 0 .. K-1 at index i (the first such) is reported as bad[0] = -1 - i, unless bad[0]
// already names a refused temperature (launch_obs_ff_bad_temperature ran before): every later launch of the call then does nothing.
hipError_t launch_obs_ff_remd_walker(int32_t* work, const int32_t* in, long long B, int K, double* bad, hipStream_t st);

// ---- Z-matrix coordinates and the histograms of all columns (obs_zmat_kernels.hip; include/ti_hip.h ti_obs_zmat, ti_obs_zmat_xyz,
// ti_obs_hist_cols).  topo: order [A] (sorted atom s is the caller's atom order[s]) followed by ref [A][3] in sorted numbering, both
// validated on the host (zmat_check_topology): every slot that is read names an earlier sorted atom.
constexpr int ZMAT_MAX_ATOMS = 32;          // 1536 A bytes of LDS per 64 molecules: 48 KB
constexpr int HIST_COLS_MAX = 128;
struct ZmatParams {
    const float* x;                         // [B][A][3], the caller's atom numbering
    long long B; int A;
    const int32_t* topo;                    // [A + 3 A]
    float* z;                               // [B][A - 1][3]: (d, a, t) of sorted atom s in row s - 1
};
struct ZmatXyzParams {
    const float* z;                         // [B][A - 1][3]
    long long B; int A;
    const int32_t* topo;
    float* x;                               // [B][A][3], the caller's atom numbering
    double* logdet;                         // [B] or NULL
    uint8_t* valid;                         // [B] or NULL
};
hipError_t launch_obs_zmat(const ZmatParams& p, hipStream_t st);
hipError_t launch_obs_zmat_xyz(const ZmatXyzParams& p, hipStream_t st);
// over the entries with keep[i] != 0: out[0] = largest finite logw (-inf: none; logw NULL: 0), out[1] = smallest index of a non-finite
// logw as a double (+inf: none), out[2] = their number; partial: [OBS_MAX_BLOCKS][3]
hipError_t launch_obs_keep_max(double* out, double* partial, const float* logw, const uint8_t* keep, long long B, hipStream_t st);
// out[0] = sum of exp(logw - m) over the entries with keep[i] != 0; partial: [OBS_MAX_BLOCKS]
hipError_t launch_obs_keep_sum(double* out, double* partial, const float* logw, const uint8_t* keep, double m, long long B, hipStream_t st);
// out [K][n_bins + 3]: launch_obs_whist of every column c of values [B][K] on [lo[c], hi[c]) in one launch, weights exp(logw - m) / tot
// (logw NULL: 1 / tot), 0 where keep (may be NULL) is 0; lo, hi: device [K]; partial: [K][OBS_MAX_BLOCKS][n_bins + 3]
hipError_t launch_obs_whist_cols(double* out, double* partial, const float* values, int K, const float* logw, const uint8_t* keep, double m,
                                 double tot, long long B, int n_bins, const double* lo, const double* hi, hipStream_t st);

// ---- bootstrap (obs_boot_kernels.hip; include/ti_hip.h ti_obs_bootstrap)
enum { BOOT_SRC_PHILOX = 0, BOOT_SRC_INDEX = 1, BOOT_SRC_IDENTITY = 2 };
struct BootParams {
    const float* v;                         // [n_pop] the population: logw itself, or the survivors of the once-only filter
    long long n_pop, n_draw;                // draws per resample; IDENTITY: n_draw == n_pop
    int source;                             // BOOT_SRC_*: where the indices of a resample come from
    const int32_t* idx;                     // [rows][n_draw] (INDEX)
    int estimator, filter;                  // TI_BOOT_*; filter != 0: every row is filtered by its own quartiles
    double k, m;                            // IQR multiple; the shift of the weights (max logw of the whole sample)
    uint64_t seed; long long first;         // PHILOX: row r is global resample first + r
    double* est;                            // [rows] estimates (NaN: nothing kept)
    double* kept;                           // [rows] kept counts (exact in fp64), may be NULL
    double* bounds;                         // [2] filter bounds of the (single) row, may be NULL
    int* flag;                              // set to 1 by an explicit index outside 0..n_pop-1 (which is then not followed)
};
// one 256-thread group per row
hipError_t launch_obs_boot(const BootParams& p, long long n_rows, hipStream_t st);
// out[0 .. *n_out) = the v[i] with bounds[0] < value(v[i]) < bounds[1] in index order (value: v itself if mean, else exp(v - m))
hipError_t launch_obs_boot_compact(float* out, double* n_out, const float* v, long long n, int mean, double m, const double* bounds, hipStream_t st);

// ---- RFF Gram matrices of resamples (obs_gram_kernels.hip; include/ti_hip.h ti_obs_rff_gram)
constexpr long long GRAM_SEG = 8192;        // draws per (row, segment) workgroup; fixed, so a row's sums do not depend on the launch
inline int gram_pad(int p) { return (p + 15) / 16 * 16; }
struct GramParams {
    BootParams draw;                        // the row's draws: source, idx, n_pop, n_draw, seed, first, flag (the rest is not read)
    const double* z;                        // [n_pop][2 P] feature table (cos | sin), P = gram_pad(p)
    const double* w;                        // [n_pop] weights, NULL: 1
    int T;                                  // P / 16
    long long nseg;                         // ceil(n_draw / GRAM_SEG)
    double* part;                           // [rows][nseg][T (T + 1) / 2][2][256] partial tiles
};
// z [n][2 P], w [n] = exp(logw - *mx) (logw == NULL: w is not written) of x [n] rows of d floats `stride` apart and omega [d][p]
hipError_t launch_obs_gram_features(double* z, double* w, const float* x, long long stride, long long n, int d, int p, const double* omega,
                                    const float* logw, const double* mx, hipStream_t st);
// one 256-thread group per (row, segment); then out [n_rows][p][p][2] = the partials added in segment order, mirrored
hipError_t launch_obs_gram(const GramParams& g, long long n_rows, hipStream_t st);
// the blocked pass of ti_obs_rff_gram_wide, 8 < g.T <= 64: one group per (row, segment, pair of 8-tile column panels I <= J); it
// fills the same partial-tile layout, so launch_obs_gram_reduce follows it unchanged
constexpr int GRAM_WIDE_MAX_P = TI_GRAM_WIDE_MAX_P;
hipError_t launch_obs_gram_wide(const GramParams& g, long long n_rows, hipStream_t st);
hipError_t launch_obs_gram_reduce(double* out, const double* part, long long n_rows, long long nseg, int p, hipStream_t st);

// ---- batched Hermitian eigensolver and the gEDMD algebra around it (obs_eig_kernels.hip; include/ti_hip.h ti_obs_eigh, ti_obs_gedmd_spectrum)
constexpr int EIG_MAX_N = TI_EIGH_MAX_N, EIG_MAX_SWEEPS = 64;
// one 256-thread group per matrix: a [n_mat] matrices mat_stride doubles apart, row stride ld complex entries, of order n -- or of
// order nvec [i] <= n (0: the matrix is skipped, status 0); w [n_mat][ldo] ascending, v [n_mat][ldo][ldo][2] or NULL;
// status [i]: the sweep count, -1 non-finite input, EIG_MAX_SWEEPS + 1 still rotating after the cap
hipError_t launch_obs_eigh(const double* a, long long mat_stride, int ld, int n, const int* nvec, double* w, double* v, int ldo, int* status,
                           long long n_mat, hipStream_t st);
// rmat [n_mat][p][p][2] (upper triangle of order rank [i]) = the Hermitian part of L^H ((coef K) o G) L from the eigenpairs (w1, u1) of G
hipError_t launch_obs_gedmd_reduce(const double* gram, const double* w1, const double* u1, const int* status1, const double* kmat, double coef,
                                   double tol, int nev, int p, double* rmat, int* rank, long long n_mat, hipStream_t st);
// ev [n_mat][nev], vec [n_mat][p][nev][2] or NULL from the eigenpairs (w2, v2) of rmat
hipError_t launch_obs_gedmd_back(const double* w1, const double* u1, const double* w2, const double* v2, const int* status2, const int* rank,
                                 int nev, int p, double* ev, double* vec, long long n_mat, hipStream_t st);

// ---- blocked eigensolver from global memory and the wide gEDMD algebra (obs_eig_wide_kernels.hip; include/ti_hip.h ti_obs_eigh_wide,
// ti_obs_gedmd_spectrum_wide)
constexpr int EIGW_MAX_N = TI_EIGH_WIDE_MAX_N, EIGW_BLK = 32, EIGW_PAIR = 2 * EIGW_BLK;
// the one statement of the launch rule (ti_obs_eigh_wide_launch_max): A and V of a launch stay within 2 GiB, 512 matrices at the most
inline long long eigw_launch_max(int n)
{
    if (n < 1 || n > EIGW_MAX_N) return 0;
    const long long fit = ((long long)1 << 31) / (32LL * n * n);
    return fit < 512 ? fit : 512;
}
inline int eigw_slots(int n) { const int nb = (n + EIGW_BLK - 1) / EIGW_BLK; return nb + (nb & 1); }      // mb: block slots of the tournament
// The work set of one launch of n_mat matrices of order n (row stride n), or of order nvec [i] <= n (below 65: the matrix is skipped).
// status [i]: 0 while iterating, then the outer sweep count, -1 non-finite input, EIG_MAX_SWEEPS + 1 still rotating after the cap,
// -2 skipped (eigw_finish turns it into 0)
struct EigWide {
    int n; const int* nvec; long long n_mat;
    double *A, *V;                          // [n_mat][n][n][2]
    double *U, *S;                          // [n_mat][eigw_slots(n) / 2][64][64][2]: the rotations and the swept block of every pair of a round
    double* thr;                            // [n_mat]
    int *rot, *prot, *status;               // [n_mat] something rotated this sweep, [n_mat][eigw_slots(n) / 2] per pair of the round, [n_mat]
};
// A, V = I, thr, status from a [n_mat] matrices mat_stride doubles apart with row stride lda
hipError_t launch_eigw_init(const EigWide& e, const double* a, long long mat_stride, int lda, hipStream_t st);
// round r of an outer sweep: the pair visits, then the column updates of A and V, then the row updates of A
hipError_t launch_eigw_round(const EigWide& e, int r, hipStream_t st);
// end of outer sweep `sweep`: a matrix that did not rotate gets status = sweep, one still rotating at the cap EIG_MAX_SWEEPS + 1
hipError_t launch_eigw_sweep_end(const EigWide& e, int sweep, hipStream_t st);
// w [n_mat][ldo] ascending and v [n_mat][ldo][ldo][2] (or NULL) of the matrices that converged
hipError_t launch_eigw_finish(const EigWide& e, double* w, double* v, int ldo, hipStream_t st);
// s [n_mat][p], rank, L [n_mat][p][p][2] (columns < rank) from the eigenpairs (w1, u1) of G; nv_narrow / nv_wide [i] = rank where the
// second solve of matrix i is ti_obs_eigh's / the blocked one, else 0; live [i] = 1 where T and R are to be formed; a kept s of 0 puts
// NaN into rmat [i][0][0]
hipError_t launch_eigw_gedmd_rank(const double* w1, const double* u1, const int* status1, double tol, int nev, int p, double* s, double* L,
                                  double* rmat, int* rank, int* nv_narrow, int* nv_wide, int* live, long long n_mat, hipStream_t st);
// T = ((coef K) o G) L, then the upper triangle of the Hermitian part of L^H T into rmat (row stride p)
hipError_t launch_eigw_gedmd_reduce(const double* gram, const double* kmat, double coef, const double* L, const int* rank, const int* live,
                                    int p, double* T, double* rmat, long long n_mat, hipStream_t st);
// ev, vec as launch_obs_gedmd_back; st2a + st2b is the status of the second solve (one of them is 0)
hipError_t launch_eigw_gedmd_back(const double* L, const double* w2, const double* v2, const int* st2a, const int* st2b, const int* rank,
                                  int nev, int p, double* ev, double* vec, long long n_mat, hipStream_t st);

// ---- TICA (obs_tica_kernels.hip; include/ti_hip.h ti_obs_tica_moments, ti_obs_tica_fit, ti_obs_tica_transform)
constexpr long long TICA_SEG = 8192;        // pairs per (lag, segment) workgroup; fixed, so a lag's sums do not depend on the launch
constexpr int TICA_MAX_LAGS = TI_TICA_MAX_LAGS;
inline int tica_tiles(int T) { return T * (T + 1) + T * T + 2 * T; }      // 16 x 16 tiles of a segment's partial: Sxx, Syy, Sxy, sum X, sum Y
inline long long tica_feature_blocks(long long n, int encode, int D) { return (n * (encode ? D / 2 : D) + 255) / 256; }
struct TicaParams {                         // one contraction launch over n_lag lags
    const double* f;                        // [n][D] feature table
    const long long* traj_off;              // [n_traj + 1]
    const long long* cum;                   // [n_lag][n_traj + 1] cumulative pair counts of the launch's lags
    int n_traj, n_lag;
    int lag[TICA_MAX_LAGS];
    int seg_off[TICA_MAX_LAGS + 1];         // first workgroup of lag l; [n_lag]: the grid
    double* part;                           // [seg_off[n_lag]][tica_tiles(T)][256] partial tiles
};
// f [n][D] and first_bad[0] = the smallest row with a non-finite value (LLONG_MAX: none); bad [tica_feature_blocks] is scratch
hipError_t launch_tica_features(double* f, long long* bad, long long* first_bad, const float* x, long long stride, long long cstride, long long n,
                                int K, int encode, int D, hipStream_t st);
// one 256-thread group per (lag, segment); then sum [n_lag][2][d], cov [n_lag][3][d][d] = the partials added in segment order
hipError_t launch_tica_moments(const TicaParams& g, int T, double* sum, double* cov, int d, hipStream_t st);
// the model algebra around the two solves of launch_obs_eigh, one group per lag
hipError_t launch_tica_fit_prep(const long long* count, const double* sum, const double* cov, int d, double* mean, double* a, double* c0t, int* flag,
                                int n_lag, hipStream_t st);
hipError_t launch_tica_fit_reduce(const double* w1, const double* v1, const int* status1, const double* c0t, double epsilon, int d, double* lmat,
                                  double* rmat, int* rank, int n_lag, hipStream_t st);
hipError_t launch_tica_fit_back(const double* lmat, const double* w2, const double* v2, const int* rank, int d, int dim, int scaling, double* ev,
                                double* comp, int n_lag, hipStream_t st);
// out [n_lag][B][dim] fp32
hipError_t launch_tica_transform(float* out, const float* x, long long stride, long long cstride, long long B, int K, int encode, int d, int dim,
                                 const double* mean, const double* comp, int n_lag, hipStream_t st);

// ---- velocity loss (vloss_kernels.hip; include/ti_hip.h ti_painn_vloss, ti_adw_vloss and their _interp twins)
constexpr int VLOSS_TILE = 1024;            // rows per tile of the batch-wide sums: fixed, so a sum does not depend on the launch
inline long long vloss_tiles(long long n) { return (n + VLOSS_TILE - 1) / VLOSS_TILE; }
struct VlossParams {
    int kind, gamma, center; double a;      // TI_VLOSS_*, TI_GAMMA_*, TI_CENTER_*
    long long B; int m, A;                  // m floats per molecule / row; A atoms (adw: 1), m = A * (m / A) components per atom
    const float *x0, *x1;                   // [B][m]
    const float* t;                         // [B]
    const float* z_in;                      // [B][m] or NULL: drawn
    uint64_t seed; long long traj0; int draw;
    float* z;                               // [B][m] the noise used (STANDARD)
    double* raw;                            // [2][B][m] uncentred states (centre BATCH / MOLECULE)
    const double* colsum;                   // [2][m / A] column sums of raw over the B A rows (BATCH)
    float* xt;                              // the plus half [B][m]; the minus half starts `half` floats behind it
    const float* b;                         // the drift on xt, laid out like xt
    long long half;                         // B m, or more when pad molecules sit between the halves (api_vloss.hip)
    double* loss;                           // [B]
};
// t [B] from the Philox word of molecule traj0 + b (include/ti_hip.h: TI_TDIST_UNIFORM / BETA_HALF / BETA_2_1)
hipError_t launch_vloss_draw_t(float* t, int t_dist, uint64_t seed, long long traj0, int draw, long long B, hipStream_t st);
// stage one, first pass: z and xt (TI_CENTER_NONE) or raw; second pass (the other centrings): xt from raw
hipError_t launch_vloss_interp(const VlossParams& p, hipStream_t st);
hipError_t launch_vloss_center(const VlossParams& p, hipStream_t st);
// out [ncol] = the sums of v [n rows][ncol] over the rows: tiles of VLOSS_TILE rows in row order into partial [tiles][ncol], then the
// tiles in order; ncol <= 16
hipError_t launch_vloss_colsum(double* out, double* partial, const double* v, long long n, int ncol, hipStream_t st);
// loss [B] from (x0, x1, t, z, b) of p
hipError_t launch_vloss_reduce(const VlossParams& p, hipStream_t st);
// out[0] = the smallest index of a non-finite loss as a double (+inf: none)
hipError_t launch_vloss_first_bad(double* out, const double* loss, long long B, hipStream_t st);
// out [n][2] = (sum of loss, count) of the rows with min(floor(t n), n - 1) == k, in index order
hipError_t launch_vloss_tbins(double* out, const double* loss, const float* t, long long B, int n, hipStream_t st);

}  // namespace ti
