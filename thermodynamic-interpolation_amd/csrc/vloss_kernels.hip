// vloss_kernels.hip -- the velocity loss of the stochastic-interpolant objective (include/ti_hip.h ti_painn_vloss, ti_adw_vloss): the
// time draws, the antithetic states of the interpolant with their centring, the per-molecule reduction of the drift against the
// interpolant's velocity, and the batch-wide sums (column means of the states, the mean loss, the time profile).  Elementwise and
// reduction work in fp64 on fp32 inputs, bound by memory; the drift between the two stages is the existing per-molecule-time path.
// No atomics: a batch-wide sum is taken over tiles of VLOSS_TILE rows in row order and over the tiles in order, each by the fixed
// tree of block_sum, so it is a function of the values and their number only -- not of the launch.
// gamma, gamma' and the z draw are vloss_device.hpp's, shared with the trainers; the states, the centring and the reduction have
// their bodies in vloss_state_body.inc, which the molecule trainer's per-molecule graphs include as well.
#include "vloss_device.hpp"

namespace ti {

namespace {

constexpr int VL_BLOCK = 256;
constexpr int VL_ROWS_PER_THREAD = VLOSS_TILE / VL_BLOCK;

// the sum of one value per thread of a VL_BLOCK-thread block, valid in thread 0: a fixed tree over the thread index
__device__ __forceinline__ double block_sum(double v, double* sm)
{
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = VL_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(VL_BLOCK) void vloss_draw_t_kernel(float* __restrict__ t, int t_dist, uint64_t seed, long long traj0, int draw,
                                                                long long B)
{
    const long long b = (long long)blockIdx.x * VL_BLOCK + threadIdx.x;
    if (b >= B) return;
    const long long id = traj0 + b;
    uint32_t c[4] = {(uint32_t)id, (uint32_t)((uint64_t)id >> 32), (uint32_t)draw, TI_VLOSS_DOMAIN};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u = ((float)(c[0] >> 9) + 0.5f) * (1.0f / 8388608.0f);      // (2k + 1) / 2^24, k < 2^23: exact
    float v = u;
    if (t_dist == TI_TDIST_BETA_HALF) { const double s = sin(0.5 * VL_PI * (double)u); v = (float)(s * s); }
    else if (t_dist == TI_TDIST_BETA_2_1) v = (float)sqrt((double)u);
    t[b] = fminf(v, 0.99999994f);                                          // 1 - 2^-24
}

// the interpolant's states, their centring and the per-molecule reduction: vloss_interp_kernel, vloss_center_kernel, vloss_reduce_kernel.
// Every molecule has p.A atoms here; the molecule trainer's per-molecule graphs take the same text with atom counts of their own
#define TI_TWIN_KERNEL(stem) vloss_##stem##_kernel
#define TI_TWIN_BLOCK VL_BLOCK
#define TI_TWIN_LIVE_PARAM
#define TI_MOL_ATOMS(b) p.A
#define TI_MOL_ENTRIES(b) p.m
#define TI_PAD_ENTRY(k, b) false
#define TI_BATCH_ATOMS (double)(p.B * p.A)
#include "vloss_state_body.inc"
#undef TI_TWIN_KERNEL
#undef TI_TWIN_BLOCK
#undef TI_TWIN_LIVE_PARAM
#undef TI_MOL_ATOMS
#undef TI_MOL_ENTRIES
#undef TI_PAD_ENTRY
#undef TI_BATCH_ATOMS

// partial [tile][col] = sum of v [row][col] over the tile's rows: thread j adds rows 4j .. 4j + 3 of the tile in order.  grid (tiles, ncol)
__global__ __launch_bounds__(VL_BLOCK) void vloss_tile_sum_kernel(double* __restrict__ partial, const double* __restrict__ v, long long n, int ncol)
{
    __shared__ double sm[VL_BLOCK];
    const int col = blockIdx.y;
    const long long r0 = (long long)blockIdx.x * VLOSS_TILE + (long long)threadIdx.x * VL_ROWS_PER_THREAD;
    double s = 0.0;
    for (int k = 0; k < VL_ROWS_PER_THREAD; ++k) if (r0 + k < n) s += v[(r0 + k) * ncol + col];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) partial[(long long)blockIdx.x * ncol + col] = s;
}

// out [col] = the tile sums in order: thread j adds tiles j, j + 256, ...  grid (ncol)
__global__ __launch_bounds__(VL_BLOCK) void vloss_tile_combine_kernel(double* __restrict__ out, const double* __restrict__ partial, long long tiles, int ncol)
{
    __shared__ double sm[VL_BLOCK];
    const int col = blockIdx.x;
    double s = 0.0;
    for (long long k = threadIdx.x; k < tiles; k += VL_BLOCK) s += partial[k * ncol + col];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) out[col] = s;
}

__global__ __launch_bounds__(VL_BLOCK) void vloss_first_bad_kernel(double* __restrict__ out, const double* __restrict__ loss, long long B)
{
    __shared__ double sm[VL_BLOCK];
    double bad = HUGE_VAL;
    for (long long i = threadIdx.x; i < B; i += VL_BLOCK)
        if (!isfinite(loss[i])) bad = fmin(bad, (double)i);
    sm[threadIdx.x] = bad;
    __syncthreads();
    for (int s = VL_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmin(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sm[0];
}

// one block per bin
__global__ __launch_bounds__(VL_BLOCK) void vloss_tbins_kernel(double* __restrict__ out, const double* __restrict__ loss, const float* __restrict__ t,
                                                               long long B, int n)
{
    __shared__ double sm[VL_BLOCK];
    const int bin = blockIdx.x;
    double s = 0.0, cnt = 0.0;
    for (long long i = threadIdx.x; i < B; i += VL_BLOCK) {
        const int k = min((int)floor((double)t[i] * (double)n), n - 1);
        if (k == bin) { s += loss[i]; cnt += 1.0; }
    }
    s = block_sum(s, sm);
    cnt = block_sum(cnt, sm);
    if (threadIdx.x == 0) { out[2 * bin] = s; out[2 * bin + 1] = cnt; }
}

unsigned blocks_for(long long n) { return (unsigned)((n + VL_BLOCK - 1) / VL_BLOCK); }

}  // namespace

hipError_t launch_vloss_draw_t(float* t, int t_dist, uint64_t seed, long long traj0, int draw, long long B, hipStream_t st)
{
    hipLaunchKernelGGL(vloss_draw_t_kernel, dim3(blocks_for(B)), dim3(VL_BLOCK), 0, st, t, t_dist, seed, traj0, draw, B);
    return hipGetLastError();
}

hipError_t launch_vloss_interp(const VlossParams& p, hipStream_t st)
{
    hipLaunchKernelGGL(vloss_interp_kernel, dim3(blocks_for(p.B * p.m)), dim3(VL_BLOCK), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_vloss_center(const VlossParams& p, hipStream_t st)
{
    hipLaunchKernelGGL(vloss_center_kernel, dim3(blocks_for(p.B * p.m), p.kind == TI_VLOSS_ONE_SIDED ? 1 : 2), dim3(VL_BLOCK), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_vloss_colsum(double* out, double* partial, const double* v, long long n, int ncol, hipStream_t st)
{
    const long long tiles = vloss_tiles(n);
    hipLaunchKernelGGL(vloss_tile_sum_kernel, dim3((unsigned)tiles, ncol), dim3(VL_BLOCK), 0, st, partial, v, n, ncol);
    hipLaunchKernelGGL(vloss_tile_combine_kernel, dim3(ncol), dim3(VL_BLOCK), 0, st, out, partial, tiles, ncol);
    return hipGetLastError();
}

hipError_t launch_vloss_reduce(const VlossParams& p, hipStream_t st)
{
    hipLaunchKernelGGL(vloss_reduce_kernel, dim3(blocks_for(p.B)), dim3(VL_BLOCK), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_vloss_first_bad(double* out, const double* loss, long long B, hipStream_t st)
{
    hipLaunchKernelGGL(vloss_first_bad_kernel, dim3(1), dim3(VL_BLOCK), 0, st, out, loss, B);
    return hipGetLastError();
}

hipError_t launch_vloss_tbins(double* out, const double* loss, const float* t, long long B, int n, hipStream_t st)
{
    hipLaunchKernelGGL(vloss_tbins_kernel, dim3(n), dim3(VL_BLOCK), 0, st, out, loss, t, B, n);
    return hipGetLastError();
}

}  // namespace ti
