// painn_update_kernel.hpp -- what the units that build the update kernel body (painn_update_kernel_body.inc) share: painn_kernels.hip
// (the builds that park v_eff in dvacc) and painn_update_keep.hip (their twins that keep it in registers).
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>

namespace ti {

struct UV {                                         // per-layer vector block in LDS, x F floats
    static constexpr int B0 = 0, G0 = 1, BE0 = 2, B1 = 3, G1 = 4, BE1 = 5, B2 = 6 /* 3F: gates | scale | add */, PB0 = 9, COUNT = 10;
};

// weight chunks per barrier.  4 (64 KB in flight per workgroup) was tried for the latency regime: no change (A = 9, B = 12: 59 vs 60 us),
// the stream of a lone workgroup runs at the ~12 B/clk a CU gets from beyond L2, not at the number of bytes in flight
// (the fp16 storage mode's hi-only chunks are half the size: four per barrier at F = 128, same LDS bytes)
__host__ __device__ constexpr int update_superchunk(int NB, bool H16) { return H16 && NB == 4 ? 4 : 2; }
__host__ __device__ constexpr int update_chunk4(int NB, bool H16) { return (H16 ? 128 : 256) * NB; }

static inline size_t update_lds_bytes(int NB, bool h16) { return 2 * update_superchunk(NB, h16) * (size_t)update_chunk4(NB, h16) * 16 + 10 * (size_t)32 * NB * 4; }

}  // namespace ti
