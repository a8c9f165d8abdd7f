// ode_device.hpp -- device helpers shared by ode_kernels.hip and its ragged twins (ode_ragged_kernels.hip): the dopri5 stage
// combinations and the fixed-order sums.  One copy, so that the uniform and the ragged kernels round alike.
#pragma once

#include "ti_internal.hpp"

namespace ti {

namespace {

constexpr int RED_BLOCK = 256;

__device__ __forceinline__ float comb(const RkComb& c, long long i)
{
    float acc = c.c[0] * c.k[0][i];
    for (int j = 1; j < c.nk; ++j) acc = fmaf(c.c[j], c.k[j][i], acc);
    return acc;
}

// block sum in a fixed tree order; result valid in thread 0
__device__ __forceinline__ double block_sum(double v)
{
    __shared__ double sm[RED_BLOCK];
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = RED_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    return sm[0];
}

constexpr int TRAJ_WAVES = 4;          // trajectories per 256-thread block (one wave each)
struct Coef7 { float c[7]; };

// sum_{j<nk} (c_j dt) k_j[i]: the coefficients scaled by the trajectory's fp32 step like comb() above (beta_ij * dt in fp32)
__device__ __forceinline__ float comb_dt(float* const* k, const float* c, int nk, float dt, long long i)
{
    float acc = (c[0] * dt) * k[0][i];
    for (int j = 1; j < nk; ++j) acc = fmaf(c[j] * dt, k[j][i], acc);
    return acc;
}

// butterfly over the wave: fp addition commutes, so every lane ends with the same bits; the order is fixed
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ bool traj_wants_row(const TrajRkParams& p, int i)
{
    return p.save_every > 0 ? (i % p.save_every == 0 || i == p.n_grid - 1) : i == p.n_grid - 1;
}

}  // namespace

}  // namespace ti
