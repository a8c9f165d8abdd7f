// painn_pair_kernel.hpp -- the PAIR-MAJOR message kernel of the cPaiNN drift: SE3Message.forward (cpainn.py:263-310, reference
// /root/reference/mdqm9/thermo/ambient/models) with the filter branch evaluated once per atom pair.
//
//   h = phi([s[src] | e]) * w(enc(|x_src - x_dst|))        (cpainn.py:283-289)
//
// `w(enc(d))` depends on the edge only through its length, so the two directed edges i -> j and j -> i of a pair share it bit for bit
// (|-r| = |r|); it is 14 of the 28 F x F products the directed kernel (painn_edge_kernel.hpp) executes per edge.  Here a row block is 16
// PAIRS (ti_internal.hpp: a 4 x 4 tile of "I" atoms x "J" atoms, row 4a + b = pair (I[a], J[b])):
//   * the w branch (2 hidden layers, 5 output slices) runs once per pair;
//   * the phi branch runs for direction A (I -> J) and direction B (J -> I) in LOCK STEP against the same weight chunk: every LDS
//     fragment feeds both operand sets (r16::gemm_x2), so a chunk visit -- its LDS-DMA, its barrier share, its fragment reads -- serves
//     32 edges instead of 16.  The packed weight stream is the directed kernel's, unchanged;
//   * the per-atom sums need no masks and no slot table walk: in the flipped output layout lane (n, q) holds rows 4q + r, i.e. I slot q
//     and J slots r = 0..3.  Direction B (dst = I[q]) is an in-lane sum of the four registers; direction A (dst = J[r]) is the sum over
//     the four lane rows, two v_permlane swap levels that leave slot q' in lane row q'.  Rows of pairs that do not exist are zeroed
//     through the shared w factor (which also carries 1 / (S_phi S_w) of the one-accumulator format).
//   * Per-atom sums (ds / dv / c): one wave owns a molecule group and walks its blocks in order, so the sums of a (block, slot) go to the
//     atom's accumulator row with fire-and-forget float atomics, the first touch of a launch replacing the stale contents (acc_out,
//     painn_edge_kernel.hpp) -- no reduction pass, nothing to zero (DESIGN.md 3.6 has the variant with partial rows and a reduction
//     kernel that this replaced).  The edge state is updated in the ROW layout (the de slice with the operands the other
//     way round, like the fp16 storage mode of the directed kernel): each e row has one owner, so e += de is a 16-byte load and store
//     per lane, no atomics.
// Per 32 directed edges: 84 chunk products and 56 chunk visits instead of 112 and 112, six LayerNorm / SiLU / operand-split phases
// instead of eight.  What it costs: 4 x 4 tiles cover a complete graph of A atoms with (A - 1) / (4 * ceil((A - 1) / 4)) of their rows
// at best (pair_template.hpp: build_pair_template; 85 % for 18 atoms), and every atom's accumulators are touched from ~ (A - 1) / 4
// blocks.  The packed template (build_pair_template_packed) therefore ends with GENERAL blocks -- 16 unrelated pairs, walked by the
// GENERAL builds below in a launch of their own right after the tile launch -- and reaches 98 % for 18 atoms (36 full tiles and 3
// general blocks per group of 4 molecules instead of 45 tiles).  Where that template is SEEDED (its general rows name every atom of a
// group exactly once: the twin rows of 18 atoms) the order turns round for plain split-path batches: the general launch first, storing
// every atom's first contribution of the layer, then tile blocks that only add (the SEEDED builds below).
// Results are deterministic (one wave owns a group of molecules, fixed order); they differ from the directed kernel's by the order
// of the per-atom sums only.
#pragma once
#include "painn_edge_kernel.hpp"

namespace ti {

// weight ring (mfma_chain.hpp PipeDMA): two superchunks of two chunks (64 KB at F = 128) in every build (pair_build_exists,
// ti_internal.hpp); DESIGN.md 3.6 has the deeper ring that lost.  The 8-wave table build at F = 128 (TABLE below) walks 20 or 16 w chunks
// per row block and parks no dv sums: its LDS holds superchunks of four (128 KB), half the closing barriers of its 512 threads.
__host__ __device__ constexpr int pair_superchunk(int NB = 0, int WAVES = 0, bool TABLE = false) { return TABLE && WAVES == 8 && NB == 4 ? 4 : 2; }
// + the builds that fold the cross term (pair_folds_cross): per wave, the 12 dv sums of every lane parked across the cross-gate products.
// At F = 128 that costs the 4-wave build its second workgroup per CU (87.5 KB); it runs below 2048 groups, where a launch has at most
// two workgroups per CU to place.
// (the GENERAL builds park their eight gate / scale products per lane instead: 32 floats)
static size_t pair_lds_bytes(int NB, int WAVES, int PREC, bool TABLE = false, bool GENERAL = false)
{
    return (size_t)2 * pair_superchunk(NB, WAVES, TABLE) * edge_chunk4(NB, false) * 16 + WAVES * 256 + 21 * (size_t)32 * NB * 4 +
           (pair_folds_cross(PREC) && !TABLE ? (size_t)WAVES * (GENERAL ? 32 : 12) * 64 * 4 : 0);
}

// TABLE (layer 0 only, the split path: pair_table_build_exists): the phi branch of layer 0 does not see the coordinates, so its three
// live output slices come from the table painn_phi0_table_kernel wrote for this evaluation (painn_phi0_kernels.hip) -- per row the
// value the products here would have given, bit for bit -- and the block walks the w chunks alone (EdgeParams: phi0_tab, cls, wpad).
template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES, bool TABLE = false>
__global__ __launch_bounds__(64 * WAVES, 2 * 4 / WAVES) void painn_pair_kernel(const EdgeParams p)
#define TI_PAIR_ROWS p.rows
#define TI_PAIR_GENERAL false
#define TI_PAIR_SEEDED false
#define TI_PAIR_TAILS false
#include "painn_pair_kernel_body.inc"
#undef TI_PAIR_ROWS
#undef TI_PAIR_GENERAL
#undef TI_PAIR_SEEDED
#undef TI_PAIR_TAILS

// Per-molecule edge sets (ti_painn_set_edge_mask): p.rows holds row words PER group (painn_pack.hip: masked_rows), in which a pair absent
// from its molecule is invalid -- zeroed through the shared w factor, like a pair that does not exist.  Both directions share that
// factor, so the molecule's edge set must be symmetric (painn_host.hip checks it when the mask is set).  The slot table and the first-touch
// writes are the template's.  Instantiated in painn_pair_mask_nb*.hip.
template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES, bool TABLE = false>
__global__ __launch_bounds__(64 * WAVES, 2 * 4 / WAVES) void painn_pair_mask_kernel(const EdgeParams p)
#define TI_PAIR_ROWS (p.rows + (size_t)gi * p.nblk * 16)
#define TI_PAIR_GENERAL false
#define TI_PAIR_SEEDED false
#define TI_PAIR_TAILS false
#include "painn_pair_kernel_body.inc"
#undef TI_PAIR_ROWS
#undef TI_PAIR_GENERAL
#undef TI_PAIR_SEEDED
#undef TI_PAIR_TAILS

// The general blocks [p.n_tile, p.nblk) of a packed template (pair_template.hpp), every row adding to its own two atoms; the two kernels
// above walk the tile blocks [0, p.n_tile).  Same body, same weight stream (cyclic per row block), same e / enc / geo rows.  One kernel
// for both kinds of row words: p.row_stride is 0 with the template's shared rows and nblk * 16 with an edge mask's per-group rows.
template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES, bool TABLE = false>
__global__ __launch_bounds__(64 * WAVES, 2 * 4 / WAVES) void painn_pair_general_kernel(const EdgeParams p)
#define TI_PAIR_ROWS (p.rows + (size_t)gi * p.row_stride)
#define TI_PAIR_GENERAL true
#define TI_PAIR_SEEDED false
#define TI_PAIR_TAILS false
#include "painn_pair_kernel_body.inc"
#undef TI_PAIR_ROWS
#undef TI_PAIR_GENERAL
#undef TI_PAIR_SEEDED
#undef TI_PAIR_TAILS

// The SEEDED builds (painn_pair_kernel_body.inc): a seeded template (pair_template.hpp) on the split path, plain batches -- no edge mask,
// one species.  The general launch of a layer runs FIRST and stores each row's two contributions, every atom's first of the layer; the
// tile launch follows on the same stream and only adds.  Two launches, never one: a store followed by an atomic to the same address
// from one wave inside one kernel has no ordering (the atomics execute at the memory side); the kernel boundary orders them.
// Instantiated in painn_pair_seed_nb*.hip.
template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES, bool TABLE = false>
__global__ __launch_bounds__(64 * WAVES, 2 * 4 / WAVES) void painn_pair_seeded_kernel(const EdgeParams p)
#define TI_PAIR_ROWS p.rows
#define TI_PAIR_GENERAL false
#define TI_PAIR_SEEDED true
#define TI_PAIR_TAILS false
#include "painn_pair_kernel_body.inc"
#undef TI_PAIR_ROWS
#undef TI_PAIR_GENERAL
#undef TI_PAIR_SEEDED
#undef TI_PAIR_TAILS

template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES, bool TABLE = false>
__global__ __launch_bounds__(64 * WAVES, 2 * 4 / WAVES) void painn_pair_general_seeded_kernel(const EdgeParams p)
#define TI_PAIR_ROWS p.rows
#define TI_PAIR_GENERAL true
#define TI_PAIR_SEEDED true
#define TI_PAIR_TAILS false
#include "painn_pair_kernel_body.inc"
#undef TI_PAIR_ROWS
#undef TI_PAIR_GENERAL
#undef TI_PAIR_SEEDED
#undef TI_PAIR_TAILS

// MERGED TAILS (painn_pair_kernel_body.inc: TAILS): the seeded general launch on a template whose last general block holds r valid
// rows, r < 16 a multiple of 4 that divides 16 (pair_template.hpp: pair_template_tails; the twin rows of 18 atoms: r = 4).  One wave
// owns S = 16 / r groups, walks their full general blocks and then their S last blocks as ONE: 9 blocks per 4 groups instead of 12 at
// 18 atoms.  Storage, row words and results are those of painn_pair_general_seeded_kernel, bit for bit.  Split path only.
// Instantiated in painn_pair_tails_nb*.hip.
template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES, bool TABLE = false>
__global__ __launch_bounds__(64 * WAVES, 2 * 4 / WAVES) void painn_pair_general_tails_kernel(const EdgeParams p)
#define TI_PAIR_ROWS p.rows
#define TI_PAIR_GENERAL true
#define TI_PAIR_SEEDED true
#define TI_PAIR_TAILS true
#include "painn_pair_kernel_body.inc"
#undef TI_PAIR_ROWS
#undef TI_PAIR_GENERAL
#undef TI_PAIR_SEEDED
#undef TI_PAIR_TAILS

// The visitor of the family: f(kernel, waves, LDS bytes) for every build of width NB that the values select (EVERY: all of them,
// dispatch.hpp), until one returns an error.  MASK: the masked twins (painn_pair_mask_kernel).  GENERAL: the builds of the general
// blocks (painn_pair_general_kernel, one per unmasked tile build of the split path; MASK is then false).  SEEDED: the seeded twins of
// the unmasked split-path builds, tile and general.  hipErrorInvalidValue: no such build.
template <int NB, bool MASK, bool GENERAL, bool SEEDED, class F>
static hipError_t with_pair_builds(int waves, int prec, int pos, F&& f)
{
    static_assert(!(MASK && GENERAL), "the general kernel takes masked row words through p.row_stride");
    static_assert(!(MASK && SEEDED), "an edge mask can take a general row away from its atoms: masked batches are never seeded");
    hipError_t e = hipSuccess;
    bool any = false;
    dispatch_int<4, 8>(waves, [&](auto wc) { dispatch_int<0, 1>(prec, [&](auto pc) {
        constexpr int WAVES = decltype(wc)::value, PREC = decltype(pc)::value;
        if constexpr (pair_build_exists(NB, WAVES, PREC) && (!(GENERAL || SEEDED) || pair_general_build_exists(PREC)))
            dispatch_int<POS_MIDDLE, POS_FIRST, POS_LAST, POS_ONLY, POS_FIRST_TABLE, POS_ONLY_TABLE>(pos, [&](auto oc) {
                constexpr bool FIRST = (decltype(oc)::value & 1) != 0, LAST = (decltype(oc)::value & 2) != 0, TABLE = (decltype(oc)::value & 4) != 0;
                if constexpr (!TABLE || pair_table_build_exists(NB, PREC, MASK)) {
                    any = true;
                    if (e != hipSuccess) return;
                    if constexpr (GENERAL && SEEDED) e = f(painn_pair_general_seeded_kernel<2 * NB, FIRST, LAST, PREC, WAVES, TABLE>, WAVES, pair_lds_bytes(NB, WAVES, PREC, TABLE, true));
                    else if constexpr (SEEDED) e = f(painn_pair_seeded_kernel<2 * NB, FIRST, LAST, PREC, WAVES, TABLE>, WAVES, pair_lds_bytes(NB, WAVES, PREC, TABLE));
                    else if constexpr (GENERAL) e = f(painn_pair_general_kernel<2 * NB, FIRST, LAST, PREC, WAVES, TABLE>, WAVES, pair_lds_bytes(NB, WAVES, PREC, TABLE, true));
                    else if constexpr (MASK) e = f(painn_pair_mask_kernel<2 * NB, FIRST, LAST, PREC, WAVES>, WAVES, pair_lds_bytes(NB, WAVES, PREC));
                    else e = f(painn_pair_kernel<2 * NB, FIRST, LAST, PREC, WAVES, TABLE>, WAVES, pair_lds_bytes(NB, WAVES, PREC, TABLE));
                }
            });
    }); });
    return any ? e : hipErrorInvalidValue;
}

// one feature width (ti_internal.hpp): configure every build / launch the one the call needs
template <int NB, bool MASK, bool GENERAL, bool SEEDED>
hipError_t configure_pair_unit()
{
    return with_pair_builds<NB, MASK, GENERAL, SEEDED>(EVERY, EVERY, EVERY, [](auto kernel, int, size_t lds) { return set_lds(kernel, lds); });
}
// (GENERAL: the launch over the general blocks, the same grid on the same stream: right after the tile launch, or with SEEDED right
// before it)
template <int NB, bool MASK, bool GENERAL, bool SEEDED>
hipError_t launch_pair_unit(bool first, bool last, int prec, const EdgeParams& p, hipStream_t st, bool table)
{
    if (table && !first) return hipErrorInvalidValue;
    if (p.n_tile < 0 || p.n_tile > p.nblk || ((GENERAL || SEEDED) && p.n_tile == p.nblk)) return hipErrorInvalidValue;
    // 8-wave workgroups (one weight stream per CU) for the split path once every CU gets a workgroup
    const bool wide = prec == 1 && p.n_groups >= 2048;
    return with_pair_builds<NB, MASK, GENERAL, SEEDED>(wide ? 8 : 4, prec, layer_pos(first, last) | (table ? POS_TABLE : 0), [&](auto kernel, int waves, size_t lds) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((p.n_groups + waves - 1) / waves)), dim3(64 * waves), lds, st, p);      // one wave = one group of G molecules
        return hipGetLastError();
    });
}

// the merged-tails builds of one width: the visitor, configure and launch of painn_pair_general_tails_kernel, as above
template <int NB, class F>
static hipError_t with_pair_tails_builds(int waves, int pos, F&& f)
{
    hipError_t e = hipSuccess;
    bool any = false;
    dispatch_int<4, 8>(waves, [&](auto wc) {
        constexpr int WAVES = decltype(wc)::value, PREC = TI_PREC_F16X2;
        if constexpr (pair_build_exists(NB, WAVES, PREC) && pair_general_build_exists(PREC))
            dispatch_int<POS_MIDDLE, POS_FIRST, POS_LAST, POS_ONLY, POS_FIRST_TABLE, POS_ONLY_TABLE>(pos, [&](auto oc) {
                constexpr bool FIRST = (decltype(oc)::value & 1) != 0, LAST = (decltype(oc)::value & 2) != 0, TABLE = (decltype(oc)::value & 4) != 0;
                if constexpr (!TABLE || pair_table_build_exists(NB, PREC, false)) {
                    any = true;
                    if (e == hipSuccess) e = f(painn_pair_general_tails_kernel<2 * NB, FIRST, LAST, PREC, WAVES, TABLE>, WAVES, pair_lds_bytes(NB, WAVES, PREC, TABLE, true));
                }
            });
    });
    return any ? e : hipErrorInvalidValue;
}
template <int NB>
hipError_t configure_pair_tails_unit()
{
    return with_pair_tails_builds<NB>(EVERY, EVERY, [](auto kernel, int, size_t lds) { return set_lds(kernel, lds); });
}
// one wave = one super-group of p.tail_S groups; the wave count follows the rule of the launches above, so that a layer's general and
// tile launch switch shapes at the same batch
template <int NB>
hipError_t launch_pair_tails_unit(bool first, bool last, const EdgeParams& p, hipStream_t st, bool table)
{
    if (table && !first) return hipErrorInvalidValue;
    if (p.n_tile < 0 || p.n_tile >= p.nblk || p.tail_S < 2 || p.tail_r < 4 || p.tail_r % 4 || p.tail_S * p.tail_r != 16) return hipErrorInvalidValue;
    const long long supers = (p.n_groups + p.tail_S - 1) / p.tail_S;
    return with_pair_tails_builds<NB>(p.n_groups >= 2048 ? 8 : 4, layer_pos(first, last) | (table ? POS_TABLE : 0), [&](auto kernel, int waves, size_t lds) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((supers + waves - 1) / waves)), dim3(64 * waves), lds, st, p);
        return hipGetLastError();
    });
}

}  // namespace ti
