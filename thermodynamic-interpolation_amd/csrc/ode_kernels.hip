// ode_kernels.hip -- elementwise pieces of the Runge-Kutta drivers (rollout.hpp): stage combinations, the scaled error /
// step-size norms of the adaptive solver (deterministic two-pass reductions), the quartic dense-output fit and evaluation.
//
// The adaptive solver restates torchdiffeq 0.2.5 (`dopri5`, /root/reference/ti_env.yml:14 -- third-party, not in the
// reference checkout): rk_common.py `_runge_kutta_step`, `_compute_error_ratio`, `_interp_fit`, `_interp_evaluate` and
// misc.py `_select_initial_step`, `_rms_norm`.  State arrays are fp32 like the reference's tensors; sums of squares are
// accumulated in fp64 and reduced in a fixed order, so accept / reject decisions repeat bit for bit.
//
// The second half holds the per-trajectory controller (TrajRkParams, ti_internal.hpp): one wave per trajectory for its norms and
// decisions, so a trajectory's step sizes, accept / reject decisions and dense output depend on its own state only and are the same
// bits in any batch, permutation or shard.
#include <climits>

#include "ode_device.hpp"

namespace ti {

// y = y0 + sum_j c_j k_j
__global__ void rk_combo_kernel(float* __restrict__ y, const float* __restrict__ y0, RkComb c, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = y0[i] + comb(c, i);
}

// partial[b] = sum_i ((sum_j c_j k_j[i]) / (atol + rtol max(|y0_i|, |y1_i|)))^2      (_compute_error_ratio)
__global__ __launch_bounds__(RED_BLOCK) void rk_ratio_partial_kernel(double* __restrict__ partial, const float* __restrict__ y0,
                                                                     const float* __restrict__ y1, RkComb c, float rtol, float atol, long long n)
{
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * RED_BLOCK) {
        const float tol = atol + rtol * fmaxf(fabsf(y0[i]), fabsf(y1[i]));
        const float r = comb(c, i) / tol;
        acc += (double)r * (double)r;
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// partial[b] = sum_i ((a_i - b_i) / (atol + rtol |y0_i|))^2   (b may be NULL)                (_select_initial_step)
__global__ __launch_bounds__(RED_BLOCK) void scaled_sq_partial_kernel(double* __restrict__ partial, const float* __restrict__ a,
                                                                      const float* __restrict__ b, const float* __restrict__ y0, float rtol,
                                                                      float atol, long long n)
{
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * RED_BLOCK) {
        const float scale = atol + fabsf(y0[i]) * rtol;
        const float r = (b ? a[i] - b[i] : a[i]) / scale;
        acc += (double)r * (double)r;
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(RED_BLOCK) void reduce_partials_kernel(double* __restrict__ out, const double* __restrict__ partial, int nb)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += RED_BLOCK) acc += partial[i];
    acc = block_sum(acc);
    if (threadIdx.x == 0) *out = acc;
}

// coefficients [5][n] of the quartic through (y0, f0), (y_mid), (y1, f1) on [t0, t0 + dt]   (_interp_fit)
__global__ void interp_fit_kernel(float* __restrict__ coef, const float* __restrict__ y0, const float* __restrict__ y1,
                                  const float* __restrict__ f0, const float* __restrict__ f1, RkComb mid, float dt, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a0 = y0[i], a1 = y1[i], g0 = f0[i], g1 = f1[i];
    const float ym = a0 + comb(mid, i);
    coef[i] = a0;
    coef[n + i] = dt * g0;
    coef[2 * n + i] = dt * (g1 - 4.0f * g0) - 11.0f * a0 - 5.0f * a1 + 16.0f * ym;
    coef[3 * n + i] = dt * (5.0f * g0 - 3.0f * g1) + 18.0f * a0 + 14.0f * a1 - 32.0f * ym;
    coef[4 * n + i] = 2.0f * dt * (g1 - g0) - 8.0f * (a1 + a0) + 16.0f * ym;
}

// total = c0 + x c1 + x^2 c2 + x^3 c3 + x^4 c4 in torchdiffeq's evaluation order   (_interp_evaluate)
__global__ void interp_eval_kernel(float* __restrict__ out, const float* __restrict__ coef, float x, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float total = coef[i] + x * coef[n + i];
    float xp = x;
#pragma unroll
    for (int k = 2; k < 5; ++k) { xp = xp * x; total = total + xp * coef[k * n + i]; }
    out[i] = total;
}

static inline dim3 grid1(long long n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }

hipError_t launch_rk_combo(float* y, const float* y0, const RkComb& c, long long n, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(rk_combo_kernel, grid1(n, 256), dim3(256), 0, st, y, y0, c, n);
    return hipGetLastError();
}
static int red_blocks(long long n) { return (int)std::min<long long>(RED_PARTIALS, std::max<long long>(1, (n + RED_BLOCK - 1) / RED_BLOCK)); }
hipError_t launch_rk_ratio_sumsq(double* out, double* partial, const float* y0, const float* y1, const RkComb& c, float rtol, float atol,
                                 long long n, hipStream_t st)
{
    const int nb = red_blocks(n);
    hipLaunchKernelGGL(rk_ratio_partial_kernel, dim3(nb), dim3(RED_BLOCK), 0, st, partial, y0, y1, c, rtol, atol, n);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(RED_BLOCK), 0, st, out, partial, nb);
    return hipGetLastError();
}
hipError_t launch_scaled_sumsq(double* out, double* partial, const float* a, const float* b, const float* y0, float rtol, float atol,
                               long long n, hipStream_t st)
{
    const int nb = red_blocks(n);
    hipLaunchKernelGGL(scaled_sq_partial_kernel, dim3(nb), dim3(RED_BLOCK), 0, st, partial, a, b, y0, rtol, atol, n);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(RED_BLOCK), 0, st, out, partial, nb);
    return hipGetLastError();
}
hipError_t launch_interp_fit(float* coef, const float* y0, const float* y1, const float* f0, const float* f1, const RkComb& mid, float dt,
                             long long n, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(interp_fit_kernel, grid1(n, 256), dim3(256), 0, st, coef, y0, y1, f0, f1, mid, dt, n);
    return hipGetLastError();
}
hipError_t launch_interp_eval(float* out, const float* coef, float x, long long n, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(interp_eval_kernel, grid1(n, 256), dim3(256), 0, st, out, coef, x, n);
    return hipGetLastError();
}

// ================================================================================================ per-trajectory dopri5
namespace {

// misc.py _mixed_norm of _rms_norm over the segments of trajectory b: max_s sqrt(sum_j term(s, i_j)^2 / m_s); a NaN propagates
template <typename Term>
__device__ double traj_norm(const TrajRkParams& p, long long b, int lane, Term term)
{
    double best = 0.0;
    for (int s = 0; s < p.nseg; ++s) {
        const long long m = p.seg[s].m, base = b * m;
        double acc = 0.0;
        for (long long j = lane; j < m; j += 64) {
            const double r = term(s, base + j);
            acc += r * r;
        }
        const double rms = sqrt(wave_sum(acc) / (double)m);
        best = (rms != rms || best != best) ? __longlong_as_double(0x7ff8000000000000LL) : fmax(best, rms);
    }
    return best;
}

}  // namespace

__global__ __launch_bounds__(256) void traj_init_kernel(const TrajRkParams p, int phase)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * TRAJ_WAVES + (threadIdx.x >> 6);
    if (b >= p.B) return;
    const float rtol = p.rtol, atol = p.atol;
    TrajCtl c = p.ctl[b];
    if (phase == 0) {                                   // _select_initial_step: d0, d1, h0, y + h0 f0
        const double d0 = traj_norm(p, b, lane, [&](int s, long long i) {
            const float y = p.seg[s].y[i];
            return (double)(y / (atol + fabsf(y) * rtol));
        });
        const double d1 = traj_norm(p, b, lane, [&](int s, long long i) {
            return (double)(p.seg[s].k[0][i] / (atol + fabsf(p.seg[s].y[i]) * rtol));
        });
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        const float one[1] = {1.0f};
        for (int s = 0; s < p.nseg; ++s) {
            const TrajSeg& g = p.seg[s];
            for (long long j = lane; j < g.m; j += 64) {
                const long long i = b * g.m + j;
                g.ytmp[i] = g.y[i] + comb_dt(g.k, one, 1, (float)h0, i);
            }
        }
        if (lane == 0) {
            c.h0 = h0; c.d1 = d1;
            p.ctl[b] = c;
            p.tv[b] = (float)(p.sign * (double)(float)(p.t_first + h0));
        }
    } else {                                            // d2, h1, the first step size; controller reset
        const double h0 = c.h0, d1 = c.d1;
        const double d2 = traj_norm(p, b, lane, [&](int s, long long i) {
            const TrajSeg& g = p.seg[s];
            return (double)((g.k[1][i] - g.k[0][i]) / (atol + fabsf(g.y[i]) * rtol));
        }) / h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / 5.0);
        c.dt = fmin(100.0 * h0, h1);
        c.t0 = c.t1 = p.t_first;
        c.next = 1;                                     // == n_grid for a one-point grid: nothing to integrate
        c.rows = traj_wants_row(p, 0) ? 1 : 0;          // row 0 is the initial state (the driver copies it)
        c.accepted = c.rejected = 0;
        if (lane == 0) p.ctl[b] = c;
    }
}

__global__ __launch_bounds__(256) void traj_stage_kernel(const TrajRkParams p, Coef7 c, int nk, float alpha, int alpha_one, int to_ynew, int stage0)
{
    const long long n0 = p.B * p.seg[0].m, n = n0 + (p.nseg > 1 ? p.B * p.seg[1].m : 0);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = i < n0 ? 0 : 1;
    const TrajSeg& g = p.seg[s];
    const long long e = s ? i - n0 : i, b = e / g.m;
    const TrajCtl& cl = p.ctl[b];
    const bool active = cl.next < p.n_grid;
    float* dst = to_ynew ? g.ynew : g.ytmp;
    dst[e] = active ? g.y[e] + comb_dt(g.k, c.c, nk, (float)cl.dt, e) : g.y[e];
    if (s == 0 && e == b * g.m) {                       // one thread per trajectory: its stage time
        float ti = (float)cl.t1;                        // frozen: any finite time will do (the result is never used)
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

__global__ __launch_bounds__(256) void traj_advance_kernel(const TrajRkParams p, Coef7 ce, Coef7 cm)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * TRAJ_WAVES + (threadIdx.x >> 6);
    if (b >= p.B) return;
    TrajCtl c = p.ctl[b];
    if (c.next >= p.n_grid) return;                     // frozen
    const double ts = c.t1, te = ts + c.dt;
    const float dtf = (float)c.dt, rtol = p.rtol, atol = p.atol;
    const double ratio = traj_norm(p, b, lane, [&](int s, long long i) {          // _compute_error_ratio
        const TrajSeg& g = p.seg[s];
        const float tol = atol + rtol * fmaxf(fabsf(g.y[i]), fabsf(g.ynew[i]));
        return (double)(comb_dt(g.k, ce.c, 7, dtf, i) / tol);
    });
    if (!(ratio == ratio)) {
        if (lane == 0) atomicMin(p.status + TRAJ_ST_NAN, (int)b);
        return;
    }
    if (ratio <= 1.0) {                                 // accept: quartic fit (_interp_fit), y <- y1, FSAL k0 <- k6
        for (int s = 0; s < p.nseg; ++s) {
            const TrajSeg& g = p.seg[s];
            const long long n = p.B * g.m;
            for (long long j = lane; j < g.m; j += 64) {
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
    // _optimal_step_size(dt, ratio, safety 0.9, ifactor 10, dfactor 0.2, order 5)
    c.dt = ratio == 0.0 ? c.dt * 10.0 : c.dt * fmin(10.0, fmax(0.9 / pow(ratio, 0.2), ratio < 1.0 ? 1.0 : 0.2));
    // dense output at every grid time the accepted interval reached (_interp_evaluate)
    while (c.next < p.n_grid && !(p.grid[c.next] > c.t1)) {
        if (traj_wants_row(p, c.next)) {
            const float x = (float)((p.grid[c.next] - c.t0) / (c.t1 - c.t0));
            for (int s = 0; s < p.nseg; ++s) {
                const TrajSeg& g = p.seg[s];
                const long long n = p.B * g.m;
                for (long long j = lane; j < g.m; j += 64) {
                    const long long i = b * g.m + j;
                    float total = g.coef[i] + x * g.coef[n + i];
                    float xp = x;
#pragma unroll
                    for (int k = 2; k < 5; ++k) { xp = xp * x; total = total + xp * g.coef[k * n + i]; }
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

static dim3 traj_waves(long long B) { return dim3((unsigned)((B + TRAJ_WAVES - 1) / TRAJ_WAVES)); }

hipError_t launch_traj_init(const TrajRkParams& p, int phase, hipStream_t st)
{
    if (p.B > 0) hipLaunchKernelGGL(traj_init_kernel, traj_waves(p.B), dim3(256), 0, st, p, phase);
    return hipGetLastError();
}
hipError_t launch_traj_stage(const TrajRkParams& p, const float* c, int nk, float alpha, int alpha_one, int to_ynew, int stage0, hipStream_t st)
{
    Coef7 cc{};
    for (int j = 0; j < nk; ++j) cc.c[j] = c[j];
    const long long n = p.B * p.seg[0].m + (p.nseg > 1 ? p.B * p.seg[1].m : 0);
    if (n > 0) hipLaunchKernelGGL(traj_stage_kernel, grid1(n, 256), dim3(256), 0, st, p, cc, nk, alpha, alpha_one, to_ynew, stage0);
    return hipGetLastError();
}
hipError_t launch_traj_advance(const TrajRkParams& p, const float* c_error, const float* c_mid, hipStream_t st)
{
    Coef7 ce{}, cm{};
    for (int j = 0; j < 7; ++j) { ce.c[j] = c_error[j]; cm.c[j] = c_mid[j]; }
    if (p.B > 0) hipLaunchKernelGGL(traj_advance_kernel, traj_waves(p.B), dim3(256), 0, st, p, ce, cm);
    return hipGetLastError();
}

}  // namespace ti
