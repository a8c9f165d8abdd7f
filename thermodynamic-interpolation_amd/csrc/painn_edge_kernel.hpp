// painn_edge_kernel.hpp -- the message ("edge") kernel of the cPaiNN drift and its launchers, one translation unit per
// feature width (painn_edge_nb{1,2,4,8}.hip) so that the 88 instantiations compile in parallel.
//   edge    : AddSpatialFeatures graph.py:25-33 + SE3Message.forward cpainn.py:263-310   (reference, /root/reference/mdqm9/thermo/ambient/models)
#pragma once
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "dispatch.hpp"
#include "mfma_chain.hpp"
#include "ti_internal.hpp"

namespace ti {

// ================================================================================================== edge kernel
// Per-layer vectors of the two message MLPs, copied once per workgroup into LDS (offsets in floats, F = n_features).
// Global loads of bias/gamma/beta in front of every weight chunk exposed a full memory latency 56 times per row block.
struct EV {
    static constexpr int W_B0 = 0, W_G0 = 1, W_BE0 = 2, W_B1 = 3, W_G1 = 4, W_BE1 = 5, P_G0 = 6, P_BE0 = 7, P_B1 = 8, P_G1 = 9,
                         P_BE1 = 10, P_B2 = 11, W_B2 = 16, COUNT = 21;      // x F
};

// Fire-and-forget fp32 add (global_atomic_add_f32, no return): nothing waits for the memory round trip.  Every
// accumulator element starts at zero and is only ever added to by the one wave that owns the molecule, in program
// order (an atom's <= 31 incoming edges span at most three 16-row blocks of that wave).
__device__ __forceinline__ void add_noret(float* p, float v) { unsafeAtomicAdd(p, v); }
// accumulator update: a fire-and-forget atomic either way -- exchange on the first touch, add afterwards -- so that the later adds of the
// same wave are ordered behind the replacement at L2 (a plain store takes another path)
__device__ __forceinline__ void acc_out(float* p, float v, bool first)
{
    if (first) (void)__hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else unsafeAtomicAdd(p, v);
}

// One wave = one molecule group, walked in blocks of 16 edge rows on the 16x16x4 MFMA (mfma_chain.hpp, namespace r16).
// The waves of a workgroup share the weight-chunk stream (4 or 8 of them, see below); two waves per SIMD (F <= 128) hide each other's
// LayerNorm / reduction / wait phases behind matrix work.
// PREC selects the matrix path (mfma_chain.hpp: OpSel): 0 f32 MFMA, 1 split fp16 (Opnd<NBK, true>), 2 fp16 storage mode (OpndH; the
// state tensors P, v, e are then fp16 in HBM).
// Workgroup width.  4 waves (two workgroups per CU) is the default; for large split-fp16 launches (>= 2048 groups, F <= 128)
// the launcher picks the 8-wave build: one 512-thread workgroup per CU shares one weight stream (half the LDS-DMA writes) and, at F = 128,
// the freed LDS holds 4-chunk superchunks (half the barriers; needs chunk counts % 4 == 0: 56/48/40/32) -- 1.8 % on the edge
// kernel at B >= 32k.  Small launches keep 4 waves: fatter workgroups cost the latency regime 20-60 %.  F = 256 needs the
// 512-register budget of one wave per SIMD and is always 4 waves.
// The fp16 storage mode streams hi-only chunks of half the size: at F = 128 it stages twice as many per barrier (same LDS bytes, half
// the barriers; the chunk counts 56/48/40/32 divide by 8).
__host__ __device__ constexpr int edge_superchunk(int NB, int WAVES, bool H16 = false) { return ((WAVES == 8 && NB == 4) ? 4 : 2) * (H16 && NB == 4 ? 2 : 1); }
__host__ __device__ constexpr int edge_chunk4(int NB, bool H16) { return (H16 ? 128 : 256) * NB; }            // float4 per weight chunk
// The builds of a width: 4 waves with NS = 2 or 4 destination atoms per row block at every precision; 8 waves (NS = 2 only) at
// F <= 128 -- except F = 32 in the storage mode, where a 2-chunk superchunk (4 KB) is smaller than one 16-byte lane per thread.
// The one-accumulator split format (edge_one_chain, ti_internal.hpp) at F = 256 (one wave per SIMD, operands partly in AGPRs) faulted on
// the device (memory aperture violation in its first launch) when hipcc spilled SGPRs into VGPR lanes: painn_edge_nb8.hip is compiled
// with -mllvm -amdgpu-spill-sgpr-to-vgpr=0 (build.py), which removes the fault.
__host__ __device__ constexpr bool edge_build_exists(int NB, int WAVES, int PREC, int NS)
{
    return PREC >= 0 && PREC <= 2 && (WAVES == 4 ? NS == 2 || NS == 4 : WAVES == 8 && NS == 2 && NB <= 4 && !(PREC == 2 && NB == 1));
}
template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES, int NS>
__global__ __launch_bounds__(64 * WAVES, (NBK <= 8 ? 2 * 4 / WAVES : 1)) void painn_edge_kernel(const EdgeParams p)
#define TI_ROWS_GROUP (gi - mg * p.parts)
#include "painn_edge_kernel_body.inc"
#undef TI_ROWS_GROUP

// Per-molecule edge sets (ti_painn_set_edge_mask): p.rows holds row words PER (group, part) (painn_pack.hip: masked_rows), in which a
// template row whose edge is absent from its molecule has slot 63 -- weight 0 in the per-atom sums, like a padding row.  The slot
// table and with it the first-touch writes are the template's, so an atom without a present incoming edge ends with zero sums.  The
// same multipliers as painn_edge_kernel: an all-ones mask gives its bits exactly.  Instantiated in painn_edge_mask_nb*.hip.
template <int NBK, bool FIRST, bool LAST, int PREC, int WAVES, int NS>
__global__ __launch_bounds__(64 * WAVES, (NBK <= 8 ? 2 * 4 / WAVES : 1)) void painn_edge_mask_kernel(const EdgeParams p)
#define TI_ROWS_GROUP (int)gi                  /* 32-bit group index: the 64-bit one cost the F = 256 kernels spills */
#include "painn_edge_kernel_body.inc"
#undef TI_ROWS_GROUP

// edge kernel LDS: two superchunks of two weight chunks, per-wave edge_dir scratch (4 waves x 16 rows x 16 B), layer vectors
static size_t edge_lds_bytes(int NB, int WAVES, bool h16) { return 2 * edge_superchunk(NB, WAVES, h16) * (size_t)edge_chunk4(NB, h16) * 16 + WAVES * 256 + 21 * (size_t)32 * NB * 4; }


// Where a message block stands among the layers, as one value to dispatch on: the kernels' (FIRST, LAST) = (pos & 1, pos & 2)
// (+ POS_TABLE: the pair kernel's layer-0 builds that read the phi table, painn_pair_kernel.hpp)
enum LayerPos { POS_MIDDLE = 0, POS_FIRST = 1, POS_LAST = 2, POS_ONLY = 3, POS_TABLE = 4, POS_FIRST_TABLE = 5, POS_ONLY_TABLE = 7 };
inline int layer_pos(bool first, bool last) { return (first ? 1 : 0) | (last ? 2 : 0); }

// The visitor of the family: f(kernel, waves, LDS bytes) for every build of width NB that the values select (EVERY: all of them,
// dispatch.hpp), until one returns an error.  MASK: the masked twins (painn_edge_mask_kernel).  hipErrorInvalidValue: no such build.
template <int NB, bool MASK, class F>
static hipError_t with_edge_builds(int waves, int ns, int prec, int pos, F&& f)
{
    hipError_t e = hipSuccess;
    bool any = false;
    dispatch_int<4, 8>(waves, [&](auto wc) { dispatch_int<2, 4>(ns, [&](auto nc) { dispatch_int<0, 1, 2>(prec, [&](auto pc) {
        constexpr int WAVES = decltype(wc)::value, NS = decltype(nc)::value, PREC = decltype(pc)::value;
        if constexpr (edge_build_exists(NB, WAVES, PREC, NS))
            dispatch_int<POS_MIDDLE, POS_FIRST, POS_LAST, POS_ONLY>(pos, [&](auto oc) {
                constexpr bool FIRST = (decltype(oc)::value & 1) != 0, LAST = (decltype(oc)::value & 2) != 0;
                any = true;
                if (e != hipSuccess) return;
                if constexpr (MASK) e = f(painn_edge_mask_kernel<2 * NB, FIRST, LAST, PREC, WAVES, NS>, WAVES, edge_lds_bytes(NB, WAVES, PREC == 2));
                else e = f(painn_edge_kernel<2 * NB, FIRST, LAST, PREC, WAVES, NS>, WAVES, edge_lds_bytes(NB, WAVES, PREC == 2));
            });
    }); }); });
    return any ? e : hipErrorInvalidValue;
}

// one feature width (ti_internal.hpp): configure every build / launch the one the call needs
template <int NB, bool MASK>
hipError_t configure_edge_unit()
{
    return with_edge_builds<NB, MASK>(EVERY, EVERY, EVERY, EVERY, [](auto kernel, int, size_t lds) { return set_lds(kernel, lds); });
}
template <int NB, bool MASK>
hipError_t launch_edge_unit(bool first, bool last, int prec, const EdgeParams& p, hipStream_t st)
{
    if (p.max_slots > EDGE_MAX_SLOTS) return hipErrorInvalidValue;          // build_templates never produces such a block
    // 8-wave workgroups: split-fp16 path only (the f32 path is matrix-bound and loses 4 % to the wider barriers), enough groups to
    // fill every CU, and at most two destination atoms per row block (the only form the wide build is instantiated for)
    const bool wide = prec != 0 && p.n_groups >= 2048 && p.max_slots <= 2 && edge_build_exists(NB, 8, prec, 2);
    return with_edge_builds<NB, MASK>(wide ? 8 : 4, p.max_slots <= 2 ? 2 : 4, prec, layer_pos(first, last), [&](auto kernel, int waves, size_t lds) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((p.n_groups + waves - 1) / waves)), dim3(64 * waves), lds, st, p);      // one wave (= one group or part) each
        return hipGetLastError();
    });
}

}  // namespace ti
