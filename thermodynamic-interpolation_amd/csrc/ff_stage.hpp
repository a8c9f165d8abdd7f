// ff_stage.hpp -- the tables of ff_device.hpp from global memory into a workgroup's LDS, for the kernels that evaluate ff_wave_forces
// (obs_ff_md_kernels.hip, obs_ff_remd_kernels.hip): 64 * FF_WAVES threads copy, the caller places the workgroup barrier.
#pragma once

#include "ff_device.hpp"

namespace ti {

namespace {

__device__ __forceinline__ FfView ff_stage_tables(const FfTablesDev& t, int32_t* s_idx, double* s_par, int32_t* s_inc)
{
    const int n_idx = t.nb + t.na + t.nt + t.np, n_par = 2 * (t.nb + t.na + t.nt) + 3 * t.np;
    for (int i = threadIdx.x; i < n_idx; i += 64 * FF_WAVES) s_idx[i] = t.idx[i];
    for (int i = threadIdx.x; i < n_par; i += 64 * FF_WAVES) s_par[i] = t.par[i];
    for (int i = threadIdx.x; i < t.inc_words; i += 64 * FF_WAVES) s_inc[i] = t.inc[i];
    FfView v;
    v.wb = s_idx; v.wa = v.wb + t.nb; v.wt = v.wa + t.na; v.wp = v.wt + t.nt;
    v.pb = s_par; v.pa = v.pb + 2 * t.nb; v.pt = v.pa + 2 * t.na; v.pp = v.pt + 2 * t.nt;
    v.inc_off = reinterpret_cast<const uint16_t*>(s_inc);
    v.inc = reinterpret_cast<const uint8_t*>(s_inc + FF_INC_OFF_WORDS);
    v.nb = t.nb; v.na = t.na; v.nt = t.nt; v.np = t.np; v.A = t.A; v.coulomb = t.coulomb;
    return v;
}

}  // namespace

}  // namespace ti
