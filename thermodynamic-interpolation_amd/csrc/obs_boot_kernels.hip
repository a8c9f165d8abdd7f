// obs_boot_kernels.hip -- bootstrap resampling of the importance-weight estimators (include/ti_hip.h ti_obs_bootstrap): ESS, TFEP and
// mean free-energy estimates of resamples of logw, with the reference's IQR outlier filter (sensititvity.py: filter_iqr).
//
// One 256-thread workgroup per resample.  Nothing is stored per resample: the group regenerates its draws from Philox4x32-10 on every
// pass over them (or reads them from an explicit index row, or walks the identity row for the point estimate).  The two quartiles of
// the filter need four order statistics of the drawn values; w = exp(v - m) is monotone in v, so they are selected on the
// order-preserving 32-bit key of the fp32 v by a 4 x 8-bit radix select with the count tables in LDS (integer LDS atomics: the counts
// do not depend on the order of the adds).  A last pass sums the kept terms: every thread adds its draws in draw order, the 256
// partial sums go through the fixed tree of ode_device.hpp.  Thread t owns the draw pairs t, t + 256, ... whatever the source of the
// draws, so the estimate of an index row is a function of the row, the data and the mode only.  No global atomics, no
// floating-point atomics.  Arithmetic is fp64 on the fp32 inputs.
#include "boot_draw.hpp"
#include "ode_device.hpp"

namespace ti {

namespace {

constexpr double BOOT_NAN = __builtin_nan("");

// order-preserving key of a finite fp32 (-0 sorts just below +0; they are the same value)
__device__ __forceinline__ uint32_t boot_key(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float boot_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }

__device__ __forceinline__ double boot_value(float v, bool mean, double m) { return mean ? (double)v : exp((double)v - m); }

// est[r], kept[r] of resample r = blockIdx.x (global resample first + r); bounds (2 doubles, may be NULL): the filter bounds used
__global__ __launch_bounds__(RED_BLOCK) void obs_boot_kernel(BootParams p)
{
    __shared__ unsigned hist[4][256];
    __shared__ uint32_t prefix[4];
    __shared__ long long rank[4];
    __shared__ int alias[4];
    const int tid = threadIdx.x;
    const long long row = blockIdx.x, nd = p.n_draw, npair = (nd + 1) / 2;
    const uint64_t R = (uint64_t)p.first + (uint64_t)row;
    const float* __restrict__ pop = p.v;
    const bool mean = p.estimator == TI_BOOT_MEAN;
    bool ok = true;
    double lo = 0.0, hi = 0.0;

    if (p.filter) {
        // ranks of the four order statistics: floor(h) and the entry after it for h = (nd - 1) / 4 and 3 (nd - 1) / 4
        const long long h25 = nd - 1, h75 = 3 * (nd - 1);
        if (tid < 4) {
            const long long hh = tid < 2 ? h25 : h75;
            rank[tid] = (hh >> 2) + ((tid & 1) && (hh & 3) ? 1 : 0);
            prefix[tid] = 0u;
            alias[tid] = 0;
        }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            for (int c = tid; c < 4 * 256; c += RED_BLOCK) (&hist[0][0])[c] = 0u;
            __syncthreads();
            const uint32_t p0 = prefix[0], p1 = prefix[1], p2 = prefix[2], p3 = prefix[3];
            const bool u1 = alias[1] == 1, u2 = alias[2] == 2, u3 = alias[3] == 3;
            for (long long pr = tid; pr < npair; pr += RED_BLOCK) {
                long long i0, i1;
                boot_draw_pair(p, row, R, pr, i0, i1, ok);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    if (e == 1 && 2 * pr + 1 >= nd) break;
                    const uint32_t key = boot_key(pop[e ? i1 : i0]);
                    const uint32_t top = pass == 0 ? 0u : key >> (shift + 8), dg = (key >> shift) & 255u;
                    if (top == p0) atomicAdd(&hist[0][dg], 1u);
                    if (u1 && top == p1) atomicAdd(&hist[1][dg], 1u);
                    if (u2 && top == p2) atomicAdd(&hist[2][dg], 1u);
                    if (u3 && top == p3) atomicAdd(&hist[3][dg], 1u);
                }
            }
            __syncthreads();
            if (tid < 4) {                      // the bin that holds rank[tid] among the entries that share prefix[tid]
                const unsigned* __restrict__ hh = hist[alias[tid]];
                long long cum = 0, rk = rank[tid];
                int b = 0;
                for (; b < 255; ++b) {
                    const long long cnt = hh[b];
                    if (cum + cnt > rk) break;
                    cum += cnt;
                }
                rank[tid] = rk - cum;
                prefix[tid] = (prefix[tid] << 8) | (uint32_t)b;
            }
            __syncthreads();
            if (tid == 0) {
                for (int t = 1; t < 4; ++t) {
                    int a = t;
                    for (int s = t - 1; s >= 0; --s) if (prefix[s] == prefix[t]) a = s;
                    alias[t] = a;
                }
            }
            __syncthreads();
        }
        const double xa = boot_value(boot_unkey(prefix[0]), mean, p.m), xb = boot_value(boot_unkey(prefix[1]), mean, p.m);
        const double xc = boot_value(boot_unkey(prefix[2]), mean, p.m), xd = boot_value(boot_unkey(prefix[3]), mean, p.m);
        const double q25 = xa + 0.25 * (double)(h25 & 3) * (xb - xa), q75 = xc + 0.25 * (double)(h75 & 3) * (xd - xc);
        const double iqr = q75 - q25;
        lo = q25 - p.k * iqr;
        hi = q75 + p.k * iqr;
        if (p.bounds && tid == 0) { p.bounds[0] = lo; p.bounds[1] = hi; }
    }

    double s1 = 0.0, s2 = 0.0, cnt = 0.0;
    for (long long pr = tid; pr < npair; pr += RED_BLOCK) {
        long long i0, i1;
        boot_draw_pair(p, row, R, pr, i0, i1, ok);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (e == 1 && 2 * pr + 1 >= nd) break;
            const float v = pop[e ? i1 : i0];
            const double x = boot_value(v, mean, p.m);
            if (!p.filter || (x > lo && x < hi)) {
                cnt += 1.0;
                s1 += x;
                s2 += x * x;
            }
        }
    }
    if (!ok) *p.flag = 1;                       // plain store of one value: whoever writes, the flag reads 1
    s1 = block_sum(s1);
    s2 = block_sum(s2);
    cnt = block_sum(cnt);
    if (tid == 0) {
        double est = BOOT_NAN;
        if (cnt > 0.0) est = p.estimator == TI_BOOT_ESS ? s1 * s1 / s2 : mean ? -(s1 / cnt) : -(p.m + log(s1 / cnt));
        p.est[row] = est;
        if (p.kept) p.kept[row] = cnt;
    }
}

// out[0 .. *n_out) = the entries of v [n] inside the filter bounds, in index order; one block walks v 256 entries at a time
__global__ __launch_bounds__(RED_BLOCK) void obs_boot_compact_kernel(float* __restrict__ out, double* __restrict__ n_out, const float* __restrict__ v,
                                                                    long long n, int mean, double m, const double* __restrict__ bounds)
{
    __shared__ int wsum[RED_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double lo = bounds[0], hi = bounds[1];
    long long done = 0;
    for (long long base = 0; base < n; base += RED_BLOCK) {
        const long long i = base + tid;
        float vi = 0.f;
        bool keep = false;
        if (i < n) {
            vi = v[i];
            const double x = boot_value(vi, mean != 0, m);
            keep = x > lo && x < hi;
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < RED_BLOCK / 64; ++w) { if (w < wave) off += wsum[w]; tot += wsum[w]; }
        if (keep) out[done + off + __popcll(b & ((1ull << lane) - 1ull))] = vi;
        done += tot;
        __syncthreads();
    }
    if (tid == 0) *n_out = (double)done;
}

}  // namespace

hipError_t launch_obs_boot(const BootParams& p, long long n_rows, hipStream_t st)
{
    if (n_rows > 0) hipLaunchKernelGGL(obs_boot_kernel, dim3((unsigned)n_rows), dim3(RED_BLOCK), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_obs_boot_compact(float* out, double* n_out, const float* v, long long n, int mean, double m, const double* bounds, hipStream_t st)
{
    hipLaunchKernelGGL(obs_boot_compact_kernel, dim3(1), dim3(RED_BLOCK), 0, st, out, n_out, v, n, mean, m, bounds);
    return hipGetLastError();
}

}  // namespace ti
