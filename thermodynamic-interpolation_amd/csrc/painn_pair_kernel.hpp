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
//     painn_edge_kernel.hpp) -- no reduction pass, nothing to zero (TI_PAIR_ACC_ATOMIC = 1, the default: 29.4 ms against 31.5 ms, same
//     box, for the alternative that is kept behind TI_PAIR_ACC_ATOMIC = 0: per-(block, slot) partial rows with plain stores +
//     `pair_reduce_kernel`, profiles/r03e_*).  The edge state is updated in the ROW layout (the de slice with the operands the other
//     way round, like the fp16 storage mode of the directed kernel): each e row has one owner, so e += de is a 16-byte load and store
//     per lane, no atomics.
// Per 32 directed edges: 84 chunk products and 56 chunk visits instead of 112 and 112, six LayerNorm / SiLU / operand-split phases
// instead of eight.  What it costs: 4 x 4 tiles cover a complete graph of A atoms with (A - 1) / (4 * ceil((A - 1) / 4)) of their rows
// at best (painn_pack.hip: build_pair_template; 85 % for 18 atoms), and every atom's accumulators are touched from ~ (A - 1) / 4 blocks.
// Results are deterministic (one wave owns a group of molecules, fixed order); they differ from the directed kernel's by the order
// of the per-atom sums only.
#pragma once
#include "painn_edge_kernel.hpp"

namespace ti {

__host__ __device__ constexpr bool pair_build_exists(int NB, int WAVES, int PREC) { return PREC != 2 && NB <= 4 && (WAVES == 4 || WAVES == 8); }
// weight ring (mfma_chain.hpp PipeDMA): 2-chunk superchunks, two of them (64 KB at F = 128) in both builds.  A deeper ring (the stream
// requested three superchunks ahead: TI_PAIR_NBUF = 4, the round's first choice) buys nothing -- every superchunk barrier drains the
// wave's memory queue anyway as soon as a store or an atomic is in flight -- and its index arithmetic cost the
// last-layer kernel 31 spilled registers: 26.16 ms with two buffers against 26.48 with four, same box (profiles/r03l_ring_depth.txt).
#ifndef TI_PAIR_NBUF
#define TI_PAIR_NBUF 2
#endif
__host__ __device__ constexpr int pair_superchunk() { return 2; }
__host__ __device__ constexpr int pair_ring(int WAVES) { return WAVES == 8 ? TI_PAIR_NBUF : 2; }
// + the builds that fold the cross term (pair_folds_cross): per wave, the 12 dv sums of every lane parked across the cross-gate products.
// At F = 128 that costs the 4-wave build its second workgroup per CU (87.5 KB); it runs below 2048 groups, where a launch has at most
// two workgroups per CU to place.
static size_t pair_lds_bytes(int NB, int WAVES, int PREC)
{
    return (size_t)pair_ring(WAVES) * pair_superchunk() * edge_chunk4(NB, false) * 16 + WAVES * 256 + 21 * (size_t)32 * NB * 4 +
           (pair_folds_cross(PREC) ? (size_t)WAVES * 12 * 64 * 4 : 0);
}

template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 2 * 4 / WAVES) void painn_pair_kernel(const EdgeParams p)
#define TI_PAIR_ROWS p.rows
#include "painn_pair_kernel_body.inc"
#undef TI_PAIR_ROWS

// Per-molecule edge sets (ti_painn_set_edge_mask): p.rows holds row words PER group (painn_pack.hip: masked_rows), in which a pair absent
// from its molecule is invalid -- zeroed through the shared w factor, like a pair that does not exist.  Both directions share that
// factor, so the molecule's edge set must be symmetric (painn_host.hip checks it when the mask is set).  The slot table and the first-touch
// writes are the template's.  Instantiated in painn_pair_mask_nb*.hip.
template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 2 * 4 / WAVES) void painn_pair_mask_kernel(const EdgeParams p)
#define TI_PAIR_ROWS (p.rows + (size_t)gi * p.nblk * 16)
#include "painn_pair_kernel_body.inc"
#undef TI_PAIR_ROWS

// MASK: the masked twins (painn_pair_mask_kernel), instantiated in translation units of their own (painn_pair_mask_nb*.hip)
template <int NB, int EW, int PREC, bool MASK>
static hipError_t configure_pair_prec()
{
    if constexpr (!pair_build_exists(NB, EW, PREC)) return hipSuccess;
    else if constexpr (MASK) {
    const size_t be = pair_lds_bytes(NB, EW, PREC);
    hipError_t e;
    if ((e = set_lds_edge(painn_pair_mask_kernel<2 * NB, true, false, PREC, EW>, be)) != hipSuccess) return e;
    if ((e = set_lds_edge(painn_pair_mask_kernel<2 * NB, false, false, PREC, EW>, be)) != hipSuccess) return e;
    if ((e = set_lds_edge(painn_pair_mask_kernel<2 * NB, false, true, PREC, EW>, be)) != hipSuccess) return e;
    if ((e = set_lds_edge(painn_pair_mask_kernel<2 * NB, true, true, PREC, EW>, be)) != hipSuccess) return e;
    return hipSuccess;
    } else {
    const size_t be = pair_lds_bytes(NB, EW, PREC);
    hipError_t e;
    if ((e = set_lds_edge(painn_pair_kernel<2 * NB, true, false, PREC, EW>, be)) != hipSuccess) return e;
    if ((e = set_lds_edge(painn_pair_kernel<2 * NB, false, false, PREC, EW>, be)) != hipSuccess) return e;
    if ((e = set_lds_edge(painn_pair_kernel<2 * NB, false, true, PREC, EW>, be)) != hipSuccess) return e;
    if ((e = set_lds_edge(painn_pair_kernel<2 * NB, true, true, PREC, EW>, be)) != hipSuccess) return e;
    return hipSuccess;
    }
}
template <int NB, bool MASK = false>
static hipError_t configure_pair_nb()
{
    hipError_t e;
    if ((e = configure_pair_prec<NB, 4, 0, MASK>()) != hipSuccess) return e;
    if ((e = configure_pair_prec<NB, 4, 1, MASK>()) != hipSuccess) return e;
    return configure_pair_prec<NB, 8, 1, MASK>();
}

template <int NB, int EW, int PREC, bool MASK>
static void launch_pair_p(bool first, bool last, const EdgeParams& p, hipStream_t st)
{
    if constexpr (pair_build_exists(NB, EW, PREC)) {
    const dim3 g((unsigned)((p.n_groups + EW - 1) / EW)), t(64 * EW);          // one wave = one group of G molecules
    const size_t l = pair_lds_bytes(NB, EW, PREC);
    if constexpr (MASK) {
    if (first && last) hipLaunchKernelGGL((painn_pair_mask_kernel<2 * NB, true, true, PREC, EW>), g, t, l, st, p);
    else if (first) hipLaunchKernelGGL((painn_pair_mask_kernel<2 * NB, true, false, PREC, EW>), g, t, l, st, p);
    else if (last) hipLaunchKernelGGL((painn_pair_mask_kernel<2 * NB, false, true, PREC, EW>), g, t, l, st, p);
    else hipLaunchKernelGGL((painn_pair_mask_kernel<2 * NB, false, false, PREC, EW>), g, t, l, st, p);
    } else {
    if (first && last) hipLaunchKernelGGL((painn_pair_kernel<2 * NB, true, true, PREC, EW>), g, t, l, st, p);
    else if (first) hipLaunchKernelGGL((painn_pair_kernel<2 * NB, true, false, PREC, EW>), g, t, l, st, p);
    else if (last) hipLaunchKernelGGL((painn_pair_kernel<2 * NB, false, true, PREC, EW>), g, t, l, st, p);
    else hipLaunchKernelGGL((painn_pair_kernel<2 * NB, false, false, PREC, EW>), g, t, l, st, p);
    }
    }
}
static bool pair_writes_partials() { return !TI_PAIR_ACC_ATOMIC; }
template <int NB, bool MASK = false>
static hipError_t launch_pair_nb(bool first, bool last, int prec, const EdgeParams& p, hipStream_t st)
{
    if (prec != 0 && prec != 1) return hipErrorInvalidValue;
    // 8-wave workgroups (one weight stream per CU, 4-chunk superchunks at F = 128) for the split path once every CU gets a workgroup
    const bool wide = prec == 1 && p.n_groups >= 2048;
    if (wide) launch_pair_p<NB, 8, 1, MASK>(first, last, p, st);
    else if (prec == 1) launch_pair_p<NB, 4, 1, MASK>(first, last, p, st);
    else launch_pair_p<NB, 4, 0, MASK>(first, last, p, st);
    return hipGetLastError();
}

}  // namespace ti
