// ode_ragged_kernels.hip -- ragged twins of the adaptive-solver kernels of ode_kernels.hip for mixed-species batches.
#include <climits>

#include "ode_device.hpp"

namespace ti {

// ================================================================================================ ragged twins (mixed species)
// Per-molecule atom counts (ti_painn_set_molecules): segment 0 holds 3A floats per trajectory of which the first 3 n_atoms[b] are
// real; the rest belong to pad atoms, whose drift is exactly 0.  The norms run over the real entries only -- same lanes, same order
// as the uniform kernels, so a trajectory's decisions are those of a batch that holds its species alone -- and pad entries of the
// state, the dense output and the path keep their initial values.  The uniform kernels (ode_kernels.hip) are left as they are: this is a
// translation unit of its own so that their code does not move; the small helpers are shared through ode_device.hpp.
namespace {

__device__ __forceinline__ bool is_pad(const int32_t* __restrict__ n_atoms, long long i, int m)
{
    const long long b = i / m;
    return (int)(i - b * m) >= 3 * n_atoms[b];
}

// traj_norm over the first cnt0 of segment 0's m entries (the rms divides by cnt0); other segments whole
template <typename Term>
__device__ double traj_norm_ragged(const TrajRkParams& p, long long b, int lane, long long cnt0, Term term)
{
    double best = 0.0;
    for (int s = 0; s < p.nseg; ++s) {
        const long long m = p.seg[s].m, base = b * m, cnt = s == 0 ? cnt0 : m;
        double acc = 0.0;
        for (long long j = lane; j < cnt; j += 64) {
            const double r = term(s, base + j);
            acc += r * r;
        }
        const double rms = sqrt(wave_sum(acc) / (double)cnt);
        best = (rms != rms || best != best) ? __longlong_as_double(0x7ff8000000000000LL) : fmax(best, rms);
    }
    return best;
}

}  // namespace

// rk_ratio_partial_kernel over the real entries of a [B][m] state (m = 3A): the same grid-stride order, pad entries skipped
__global__ __launch_bounds__(RED_BLOCK) void rk_ratio_partial_ragged_kernel(double* __restrict__ partial, const float* __restrict__ y0,
                                                                            const float* __restrict__ y1, RkComb c, float rtol, float atol,
                                                                            long long n, const int32_t* __restrict__ n_atoms, int m)
{
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * RED_BLOCK) {
        if (is_pad(n_atoms, i, m)) continue;
        const float tol = atol + rtol * fmaxf(fabsf(y0[i]), fabsf(y1[i]));
        const float r = comb(c, i) / tol;
        acc += (double)r * (double)r;
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(RED_BLOCK) void scaled_sq_partial_ragged_kernel(double* __restrict__ partial, const float* __restrict__ a,
                                                                             const float* __restrict__ b, const float* __restrict__ y0,
                                                                             float rtol, float atol, long long n,
                                                                             const int32_t* __restrict__ n_atoms, int m)
{
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * RED_BLOCK) {
        if (is_pad(n_atoms, i, m)) continue;
        const float scale = atol + fabsf(y0[i]) * rtol;
        const float r = (b ? a[i] - b[i] : a[i]) / scale;
        acc += (double)r * (double)r;
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void traj_init_ragged_kernel(const TrajRkParams p, int phase, const int32_t* __restrict__ n_atoms)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * TRAJ_WAVES + (threadIdx.x >> 6);
    if (b >= p.B) return;
    const float rtol = p.rtol, atol = p.atol;
    const long long cnt0 = 3LL * n_atoms[b];
    TrajCtl c = p.ctl[b];
    if (phase == 0) {
        const double d0 = traj_norm_ragged(p, b, lane, cnt0, [&](int s, long long i) {
            const float y = p.seg[s].y[i];
            return (double)(y / (atol + fabsf(y) * rtol));
        });
        const double d1 = traj_norm_ragged(p, b, lane, cnt0, [&](int s, long long i) {
            return (double)(p.seg[s].k[0][i] / (atol + fabsf(p.seg[s].y[i]) * rtol));
        });
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        const float one[1] = {1.0f};
        for (int s = 0; s < p.nseg; ++s) {
            const TrajSeg& g = p.seg[s];
            const long long cnt = s == 0 ? cnt0 : g.m;
            for (long long j = lane; j < g.m; j += 64) {
                const long long i = b * g.m + j;
                g.ytmp[i] = j < cnt ? g.y[i] + comb_dt(g.k, one, 1, (float)h0, i) : g.y[i];
            }
        }
        if (lane == 0) {
            c.h0 = h0; c.d1 = d1;
            p.ctl[b] = c;
            p.tv[b] = (float)(p.sign * (double)(float)(p.t_first + h0));
        }
    } else {
        const double h0 = c.h0, d1 = c.d1;
        const double d2 = traj_norm_ragged(p, b, lane, cnt0, [&](int s, long long i) {
            const TrajSeg& g = p.seg[s];
            return (double)((g.k[1][i] - g.k[0][i]) / (atol + fabsf(g.y[i]) * rtol));
        }) / h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / 5.0);
        c.dt = fmin(100.0 * h0, h1);
        c.t0 = c.t1 = p.t_first;
        c.next = 1;
        c.rows = traj_wants_row(p, 0) ? 1 : 0;
        c.accepted = c.rejected = 0;
        if (lane == 0) p.ctl[b] = c;
    }
}

__global__ __launch_bounds__(256) void traj_stage_ragged_kernel(const TrajRkParams p, Coef7 c, int nk, float alpha, int alpha_one, int to_ynew,
                                                                int stage0, const int32_t* __restrict__ n_atoms)
{
    const long long n0 = p.B * p.seg[0].m, n = n0 + (p.nseg > 1 ? p.B * p.seg[1].m : 0);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = i < n0 ? 0 : 1;
    const TrajSeg& g = p.seg[s];
    const long long e = s ? i - n0 : i, b = e / g.m;
    const TrajCtl& cl = p.ctl[b];
    const bool active = cl.next < p.n_grid;
    const bool live = active && (s != 0 || e - b * g.m < 3LL * n_atoms[b]);      // a pad entry copies y like a frozen trajectory
    float* dst = to_ynew ? g.ynew : g.ytmp;
    dst[e] = live ? g.y[e] + comb_dt(g.k, c.c, nk, (float)cl.dt, e) : g.y[e];
    if (s == 0 && e == b * g.m) {
        float ti = (float)cl.t1;
        if (active) {
            const double ts = cl.t1, te = ts + cl.dt;
            const float tsf = (float)ts, dtf = (float)cl.dt, tef = (float)te;
            ti = alpha_one ? nextafterf(tef, tef - 1.0f) : __fadd_rn(tsf, __fmul_rn(alpha, dtf));
            if (stage0) {
                if (!(te > ts)) atomicMin(p.status + TRAJ_ST_UNDERFLOW, (int)b);
                if ((long long)cl.accepted + cl.rejected + 1 > p.max_attempts) atomicMin(p.status + TRAJ_ST_LIMIT, (int)b);
            }
        }
        p.tv[b] = (float)(p.sign * (double)ti);
    }
}

__global__ __launch_bounds__(256) void traj_advance_ragged_kernel(const TrajRkParams p, Coef7 ce, Coef7 cm, const int32_t* __restrict__ n_atoms)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * TRAJ_WAVES + (threadIdx.x >> 6);
    if (b >= p.B) return;
    TrajCtl c = p.ctl[b];
    if (c.next >= p.n_grid) return;
    const long long cnt0 = 3LL * n_atoms[b];
    const double ts = c.t1, te = ts + c.dt;
    const float dtf = (float)c.dt, rtol = p.rtol, atol = p.atol;
    const double ratio = traj_norm_ragged(p, b, lane, cnt0, [&](int s, long long i) {
        const TrajSeg& g = p.seg[s];
        const float tol = atol + rtol * fmaxf(fabsf(g.y[i]), fabsf(g.ynew[i]));
        return (double)(comb_dt(g.k, ce.c, 7, dtf, i) / tol);
    });
    if (!(ratio == ratio)) {
        if (lane == 0) atomicMin(p.status + TRAJ_ST_NAN, (int)b);
        return;
    }
    if (ratio <= 1.0) {
        for (int s = 0; s < p.nseg; ++s) {
            const TrajSeg& g = p.seg[s];
            const long long n = p.B * g.m, cnt = s == 0 ? cnt0 : g.m;
            for (long long j = lane; j < cnt; j += 64) {
                const long long i = b * g.m + j;
                const float a0 = g.y[i], a1 = g.ynew[i], g0 = g.k[0][i], g1 = g.k[6][i];
                const float ym = a0 + comb_dt(g.k, cm.c, 7, dtf, i);
                g.coef[i] = a0;
                g.coef[n + i] = dtf * g0;
                g.coef[2 * n + i] = dtf * (g1 - 4.0f * g0) - 11.0f * a0 - 5.0f * a1 + 16.0f * ym;
                g.coef[3 * n + i] = dtf * (5.0f * g0 - 3.0f * g1) + 18.0f * a0 + 14.0f * a1 - 32.0f * ym;
                g.coef[4 * n + i] = 2.0f * dtf * (g1 - g0) - 8.0f * (a1 + a0) + 16.0f * ym;
                g.y[i] = a1;
                g.k[0][i] = g1;
            }
        }
        c.t0 = ts; c.t1 = te;
        ++c.accepted;
    } else {
        ++c.rejected;
    }
    c.dt = ratio == 0.0 ? c.dt * 10.0 : c.dt * fmin(10.0, fmax(0.9 / pow(ratio, 0.2), ratio < 1.0 ? 1.0 : 0.2));
    while (c.next < p.n_grid && !(p.grid[c.next] > c.t1)) {
        if (traj_wants_row(p, c.next)) {
            const float x = (float)((p.grid[c.next] - c.t0) / (c.t1 - c.t0));
            for (int s = 0; s < p.nseg; ++s) {
                const TrajSeg& g = p.seg[s];
                const long long n = p.B * g.m, cnt = s == 0 ? cnt0 : g.m;
                for (long long j = lane; j < g.m; j += 64) {
                    const long long i = b * g.m + j;
                    float total = g.y[i];                       // a pad entry: its state, which nothing has moved
                    if (j < cnt) {
                        total = g.coef[i] + x * g.coef[n + i];
                        float xp = x;
#pragma unroll
                        for (int k = 2; k < 5; ++k) { xp = xp * x; total = total + xp * g.coef[k * n + i]; }
                    }
                    g.out[(size_t)c.rows * n + i] = g.out_scale * total;
                }
            }
            ++c.rows;
        }
        ++c.next;
    }
    if (lane == 0) {
        p.ctl[b] = c;
        if (c.next < p.n_grid) atomicAdd(p.status + TRAJ_ST_ACTIVE, 1);
        atomicMax(p.status + TRAJ_ST_MISSING, p.total_rows - c.rows);
    }
}

static inline dim3 grid1(long long n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }
static dim3 traj_waves(long long B) { return dim3((unsigned)((B + TRAJ_WAVES - 1) / TRAJ_WAVES)); }
static int red_blocks(long long n) { return (int)std::min<long long>(RED_PARTIALS, std::max<long long>(1, (n + RED_BLOCK - 1) / RED_BLOCK)); }

__global__ __launch_bounds__(RED_BLOCK) void reduce_partials_ragged_kernel(double* __restrict__ out, const double* __restrict__ partial, int nb)
{
    double acc = 0.0;                                   // reduce_partials_kernel of ode_kernels.hip: the same fixed order
    for (int i = threadIdx.x; i < nb; i += RED_BLOCK) acc += partial[i];
    acc = block_sum(acc);
    if (threadIdx.x == 0) *out = acc;
}

hipError_t launch_rk_ratio_sumsq_ragged(double* out, double* partial, const float* y0, const float* y1, const RkComb& c, float rtol, float atol,
                                        long long n, const int32_t* n_atoms, int m, hipStream_t st)
{
    const int nb = red_blocks(n);
    hipLaunchKernelGGL(rk_ratio_partial_ragged_kernel, dim3(nb), dim3(RED_BLOCK), 0, st, partial, y0, y1, c, rtol, atol, n, n_atoms, m);
    hipLaunchKernelGGL(reduce_partials_ragged_kernel, dim3(1), dim3(RED_BLOCK), 0, st, out, partial, nb);
    return hipGetLastError();
}
hipError_t launch_scaled_sumsq_ragged(double* out, double* partial, const float* a, const float* b, const float* y0, float rtol, float atol,
                                      long long n, const int32_t* n_atoms, int m, hipStream_t st)
{
    const int nb = red_blocks(n);
    hipLaunchKernelGGL(scaled_sq_partial_ragged_kernel, dim3(nb), dim3(RED_BLOCK), 0, st, partial, a, b, y0, rtol, atol, n, n_atoms, m);
    hipLaunchKernelGGL(reduce_partials_ragged_kernel, dim3(1), dim3(RED_BLOCK), 0, st, out, partial, nb);
    return hipGetLastError();
}
hipError_t launch_traj_init_ragged(const TrajRkParams& p, int phase, const int32_t* n_atoms, hipStream_t st)
{
    if (p.B > 0) hipLaunchKernelGGL(traj_init_ragged_kernel, traj_waves(p.B), dim3(256), 0, st, p, phase, n_atoms);
    return hipGetLastError();
}
hipError_t launch_traj_stage_ragged(const TrajRkParams& p, const float* c, int nk, float alpha, int alpha_one, int to_ynew, int stage0,
                                    const int32_t* n_atoms, hipStream_t st)
{
    Coef7 cc{};
    for (int j = 0; j < nk; ++j) cc.c[j] = c[j];
    const long long n = p.B * p.seg[0].m + (p.nseg > 1 ? p.B * p.seg[1].m : 0);
    if (n > 0) hipLaunchKernelGGL(traj_stage_ragged_kernel, grid1(n, 256), dim3(256), 0, st, p, cc, nk, alpha, alpha_one, to_ynew, stage0, n_atoms);
    return hipGetLastError();
}
hipError_t launch_traj_advance_ragged(const TrajRkParams& p, const float* c_error, const float* c_mid, const int32_t* n_atoms, hipStream_t st)
{
    Coef7 ce{}, cm{};
    for (int j = 0; j < 7; ++j) { ce.c[j] = c_error[j]; cm.c[j] = c_mid[j]; }
    if (p.B > 0) hipLaunchKernelGGL(traj_advance_ragged_kernel, traj_waves(p.B), dim3(256), 0, st, p, ce, cm, n_atoms);
    return hipGetLastError();
}

}  // namespace ti
