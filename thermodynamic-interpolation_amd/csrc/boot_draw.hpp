// boot_draw.hpp -- the draws of a bootstrap resample (include/ti_hip.h ti_obs_bootstrap, "Draws"), shared by the kernels that
// resample: obs_boot_kernels.hip (weight estimators) and obs_gram_kernels.hip (RFF Gram matrices).  One definition, so that a
// resample R of a seed is the same multiset of population indices in both.
#pragma once
#include "adw_device.hpp"
#include "ti_internal.hpp"

namespace ti {

namespace {

// population indices of the draws 2p and 2p + 1 of the group's resample (i1 is not used when 2p + 1 == n_draw).  ok = false: an
// explicit index outside the population; it is replaced by 0, so nothing is read out of bounds, and the call is refused afterwards.
__device__ __forceinline__ void boot_draw_pair(const BootParams& p, long long row, uint64_t R, long long pr, long long& i0, long long& i1, bool& ok)
{
    const long long j = 2 * pr;
    if (p.source == BOOT_SRC_IDENTITY) {
        i0 = j; i1 = j + 1;
    } else if (p.source == BOOT_SRC_INDEX) {
        const int32_t* __restrict__ ix = p.idx + row * p.n_draw + j;
        i0 = ix[0];
        i1 = j + 1 < p.n_draw ? ix[1] : 0;
        if (i0 < 0 || i0 >= p.n_pop) { i0 = 0; ok = false; }
        if (i1 < 0 || i1 >= p.n_pop) { i1 = 0; ok = false; }
    } else {
        uint32_t c[4] = {(uint32_t)pr, (uint32_t)R, (uint32_t)(R >> 32), TI_BOOT_DOMAIN};
        // the key words in vector registers: left uniform, the ten round keys are hoisted into 20 scalar registers and the kernel spills
        uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
        asm volatile("" : "+v"(k0), "+v"(k1));
        philox4x32_10(c, k0, k1);
        i0 = (long long)__umul64hi(((uint64_t)c[1] << 32) | c[0], (uint64_t)p.n_pop);
        i1 = (long long)__umul64hi(((uint64_t)c[3] << 32) | c[2], (uint64_t)p.n_pop);
    }
}

}  // namespace

}  // namespace ti
