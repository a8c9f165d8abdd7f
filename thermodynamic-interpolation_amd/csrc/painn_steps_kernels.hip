// painn_steps_kernels.hip -- the kernels ti_painn_train_steps adds around the passes of a training step (include/ti_hip.h): the gather
// of a minibatch and its conditioning from the resident sets, the log entry of a forward-only step, and the best-weights rule.  All
// elementwise: no reduction, no atomics.
#include "painn_steps.hpp"

namespace ti {

namespace {

constexpr int PS_BLOCK = 256;

// thread i < 3 A B: one coordinate of both gathered sets; thread i < A B writes the conditioning of atom row i as well
__global__ __launch_bounds__(PS_BLOCK) void ptsteps_gather_kernel(const PtGather g)
{
    const long long m = 3LL * g.A, n = g.B * m, i = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long b = i / m, c = i - b * m;
    long long r0 = g.idx0 ? g.idx0[b] : b, r1 = g.idx1 ? g.idx1[b] : b;
    if (r0 < 0 || r0 >= g.n0) r0 = 0;
    if (r1 < 0 || r1 >= g.n1) r1 = 0;
    if (g.x0) g.gx0[i] = g.x0[r0 * m + c];
    g.gx1[i] = g.x1[r1 * m + c];
    if (i < g.B * g.A && g.ncond > 0) {
        const long long bb = i / g.A;
        long long q0 = g.idx0 ? g.idx0[bb] : bb, q1 = g.idx1 ? g.idx1[bb] : bb;
        if (q0 < 0 || q0 >= g.n0) q0 = 0;
        if (q1 < 0 || q1 >= g.n1) q1 = 0;
        if (g.ncond == 2) { g.cond[2 * i] = g.temp0[q0]; g.cond[2 * i + 1] = g.temp1[q1]; }
        else g.cond[i] = g.temp1[q1];
    }
}

__global__ void ptsteps_log_kernel(double* __restrict__ log, const double* __restrict__ loss_sum, double divisor)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) log[0] = loss_sum[0] / divisor;
}

// the step's loss where the optimiser will apply the step, NaN where it will skip it
__device__ __forceinline__ double best_candidate(const PtBest& b)
{
#pragma clang fp contract(off)
    const double ss = b.sumsq[0], mean = b.loss_sum[0] / b.divisor;
    return isfinite(ss) && isfinite(mean) ? mean : __longlong_as_double(0x7ff8000000000000LL);
}

__global__ __launch_bounds__(PS_BLOCK) void ptsteps_best_keep_kernel(const PtBest b)
{
    const size_t i = (size_t)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (i >= b.n) return;
    if (best_candidate(b) < b.best[0]) b.best_w[i] = b.w[i];         // a NaN compares false
}

__global__ void ptsteps_best_commit_kernel(const PtBest b)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double c = best_candidate(b);
    if (c < b.best[0]) { b.best[0] = c; b.best[1] = b.step; }
}

unsigned ps_blocks(long long n) { return (unsigned)((n + PS_BLOCK - 1) / PS_BLOCK); }

}  // namespace

hipError_t launch_ptsteps_gather(const PtGather& g, hipStream_t st)
{
    hipLaunchKernelGGL(ptsteps_gather_kernel, dim3(ps_blocks(g.B * 3 * g.A)), dim3(PS_BLOCK), 0, st, g);
    return hipGetLastError();
}

hipError_t launch_ptsteps_log(double* log, const double* loss_sum, double divisor, hipStream_t st)
{
    hipLaunchKernelGGL(ptsteps_log_kernel, dim3(1), dim3(64), 0, st, log, loss_sum, divisor);
    return hipGetLastError();
}

hipError_t launch_ptsteps_best_keep(const PtBest& b, hipStream_t st)
{
    hipLaunchKernelGGL(ptsteps_best_keep_kernel, dim3(ps_blocks((long long)b.n)), dim3(PS_BLOCK), 0, st, b);
    return hipGetLastError();
}

hipError_t launch_ptsteps_best_commit(const PtBest& b, hipStream_t st)
{
    hipLaunchKernelGGL(ptsteps_best_commit_kernel, dim3(1), dim3(64), 0, st, b);
    return hipGetLastError();
}

}  // namespace ti
