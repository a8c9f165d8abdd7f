// obs_bg_kernels.hip -- the Boltzmann-generator log-weights (include/ti_hip.h ti_obs_bg_logw): log N(z; 0, I) of every row of a batch
// of prior samples and the log-weight formed from it, the reduced energy of the generated state and the two dlogps.  One wave per
// row, FF_WAVES rows per workgroup as in obs_ff_energy_kernel.  Lane l adds the squares of components l, l + 64, ... in that order
// -- every square of an fp32 value is exact in fp64 -- and the 64 lane sums are combined by the fixed butterfly of wave_sum, so a
// row's outputs are a function of the row and m only: which wave, which workgroup and which trip computes it does not enter.  fp64
// without contraction (m * TI_BG_HALF_LOG_2PI is rounded before it is subtracted), no LDS, no barriers, no atomics.
#include "ode_device.hpp"

namespace ti {

namespace {

__global__ __launch_bounds__(64 * FF_WAVES) void obs_bg_logw_kernel(BgParams p)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long base = (long long)blockIdx.x * FF_WAVES; base < p.B; base += (long long)gridDim.x * FF_WAVES) {
        const long long b = base + wave;
        if (b >= p.B) continue;                             // no workgroup barrier below: a wave past the end just idles
        const float* __restrict__ row = p.z + b * p.m;
        double s = 0.0;
        for (int c = lane; c < p.m; c += 64) {
            const double v = (double)row[c];
            s += v * v;
        }
        s = wave_sum(s);
        if (lane != 0) continue;
        const double logpz = -(0.5 * s) - ((double)p.m * TI_BG_HALF_LOG_2PI);
        if (p.logpz) p.logpz[b] = logpz;
        if (p.logw) {
            const double u = p.u1 ? p.u1[b] : 0.0, nb = p.nd_bg ? (double)p.nd_bg[b] : 0.0, nt = p.nd_ti ? (double)p.nd_ti[b] : 0.0;
            p.logw[b] = (float)-(((u + logpz) + nb) + nt);
        }
    }
}

// the unrounded log-weight of molecule i, the expression of obs_bg_logw_kernel ahead of its rounding
__device__ __forceinline__ double bg_logw64(const BgEssParams& p, long long i)
{
#pragma clang fp contract(off)
    const double u = p.u1 ? p.u1[i] : 0.0, nb = p.nd_bg ? (double)p.nd_bg[i] : 0.0, nt = p.nd_ti ? (double)p.nd_ti[i] : 0.0;
    return -(((u + p.logpz[i]) + nb) + nt);
}

// fixed tree over the workgroup; every thread returns the result
template <typename Op>
__device__ __forceinline__ double block_all(double v, double* sm, Op op)
{
    __syncthreads();                                        // the previous reduction's reads
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = RED_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = op(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    return sm[0];
}

// One workgroup: thread t walks the kept molecules t, t + 256, ... in that order, three times -- the smallest index of a non-finite
// log-weight, the largest log-weight, then sum w and sum w^2 with w = exp(l - max) -- each pass closed by the fixed tree.  fp64
// throughout, no atomics.  out = (ess, kept count, first bad index or +inf); with a bad index the ess is not formed.
__global__ __launch_bounds__(RED_BLOCK) void obs_bg_ess_kernel(BgEssParams p)
{
#pragma clang fp contract(off)
    __shared__ double sm[RED_BLOCK];
    double bad = HUGE_VAL, mx = -HUGE_VAL, n = 0.0;
    for (long long i = threadIdx.x; i < p.B; i += RED_BLOCK) {
        if (p.keep && !p.keep[i]) continue;
        const double l = bg_logw64(p, i);
        n += 1.0;
        if (!isfinite(l)) bad = fmin(bad, (double)i);
        else mx = fmax(mx, l);
    }
    bad = block_all(bad, sm, [](double a, double b) { return fmin(a, b); });
    mx = block_all(mx, sm, [](double a, double b) { return fmax(a, b); });
    n = block_all(n, sm, [](double a, double b) { return a + b; });
    double s1 = 0.0, s2 = 0.0;
    if (bad == HUGE_VAL)
        for (long long i = threadIdx.x; i < p.B; i += RED_BLOCK) {
            if (p.keep && !p.keep[i]) continue;
            const double w = exp(bg_logw64(p, i) - mx);
            s1 += w; s2 += w * w;
        }
    s1 = block_all(s1, sm, [](double a, double b) { return a + b; });
    s2 = block_all(s2, sm, [](double a, double b) { return a + b; });
    if (threadIdx.x == 0) { p.out[0] = s1 * s1 / s2; p.out[1] = n; p.out[2] = bad; }
}

}  // namespace

hipError_t launch_obs_bg_ess(const BgEssParams& p, hipStream_t st)
{
    hipLaunchKernelGGL(obs_bg_ess_kernel, dim3(1), dim3(RED_BLOCK), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_obs_bg_logw(const BgParams& p, hipStream_t st)
{
    if (p.B < 1) return hipSuccess;
    // enough workgroups to fill the chip several times over; the result does not depend on the cut
    const long long groups = std::min<long long>((p.B + FF_WAVES - 1) / FF_WAVES, 16384);
    hipLaunchKernelGGL(obs_bg_logw_kernel, dim3((unsigned)groups), dim3(64 * FF_WAVES), 0, st, p);
    return hipGetLastError();
}

}  // namespace ti
