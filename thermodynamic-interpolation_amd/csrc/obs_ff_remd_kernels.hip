// obs_ff_remd_kernels.hip -- the exchange attempt of replica exchange (include/ti_hip.h ti_obs_ff_remd), run between two launches of
// the Langevin kernel (obs_ff_md_kernels.hip), which stays as it is.  One launch is one attempt.  One wave per pair (k, k + 1) of a
// ladder, FF_WAVES waves per workgroup, the tables staged once: the wave loads row k, evaluates it through ff_wave_forces (the body
// behind out_epot, so E_k has a frame's bits), keeps E_k, does the same for row k + 1, decides -- every lane computes the same
// decision from the same bits -- and on acceptance writes components lane and lane + 64 of both rows' positions and velocities back
// exchanged, the velocities rescaled at the positions' time (the forces of the two passes give the half kick the stored velocity
// lags by).  The energies never leave the chip.  fp64 without contraction; a pair's labels and counts are
// owned by its wave: ordinary loads and stores, no atomics.  No workgroup barrier after the tables are staged.
//
// A ladder has max(pairs, 1) waves: wave j holds the pair (par + 2 j, par + 2 j + 1), par = n % 2, if that exists.  The rungs that
// sit out an attempt (rung 0 when par == 1, rung K - 1 when K - par is odd) have their label copied to out_walker by the ladder's
// first and last wave, so a ladder of two rungs at an odd attempt still has a wave, without a pair.
#include "ff_device.hpp"
#include "ff_stage.hpp"
#include "adw_device.hpp"
#include "vloss_normal.hpp"

namespace ti {

namespace {

__global__ __launch_bounds__(64 * FF_WAVES) void obs_ff_remd_kernel(RemdParams p)
{
#pragma clang fp contract(off)
    __shared__ int32_t s_idx[FFD_IDX_WORDS];
    __shared__ double s_par[FFD_PAR_DOUBLES];
    __shared__ int32_t s_inc[FF_INC_WORDS];
    __shared__ double s_x[FF_WAVES][FFD_X_DOUBLES], s_f[FF_WAVES][FFD_X_DOUBLES], s_stage[FF_WAVES][FF_STAGE_DOUBLES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const FfView t = ff_stage_tables(p.t, s_idx, s_par, s_inc);
    __syncthreads();                                        // the only workgroup barrier: the tables
    if (p.bad_T[0] < (double)p.B) return;                   // a refused temperature or label: the host reports it, nothing is written
    const int K = p.K, par = (int)(p.attempt & 1), pairs = (K - par) / 2, per = pairs > 0 ? pairs : 1;
    const long long n_ladders = p.B / K, w = (long long)blockIdx.x * FF_WAVES + wave;
    if (w >= n_ladders * per) return;
    const long long l = w / per;
    const int j = (int)(w - l * per), k = par + 2 * j;
    const long long ra = l * K + k, rb = ra + 1;            // rb is read only when the pair exists
    if (p.out_walker && lane == 0) {                        // the rungs that sit out
        if (j == 0 && par == 1) p.out_walker[l * K] = p.walker[l * K];
        if (j == per - 1 && ((K - par) & 1)) p.out_walker[l * K + K - 1] = p.walker[l * K + K - 1];
    }
    if (k + 1 >= K) return;
    double *sx = s_x[wave], *sf = s_f[wave], *stage = s_stage[wave];
    const int m3 = 3 * t.A, c0 = lane, c1 = lane + 64;
    const bool on0 = c0 < m3, on1 = c1 < m3;
    double e[4];
    const double xa0 = on0 ? p.pos[ra * m3 + c0] : 0.0, xa1 = on1 ? p.pos[ra * m3 + c1] : 0.0;
    if (on0) sx[c0] = xa0;
    if (on1) sx[c1] = xa1;
    ff_wave_sync();
    ff_wave_forces(t, sx, sf, stage, lane, e);
    const double ea = ((e[0] + e[1]) + e[2]) + e[3];
    // half a kick of each row, (dt / 2) f / m: what the stored velocity lags behind the positions (below)
    const double half = p.dt * 0.5, m0 = on0 ? p.mass[c0 / 3] : 1.0, m1 = on1 ? p.mass[c1 / 3] : 1.0;
    const double ha0 = on0 ? half * sf[c0] / m0 : 0.0, ha1 = on1 ? half * sf[c1] / m1 : 0.0;
    ff_wave_sync();                                         // row k + 1 overwrites sx and sf
    const double xb0 = on0 ? p.pos[rb * m3 + c0] : 0.0, xb1 = on1 ? p.pos[rb * m3 + c1] : 0.0;
    if (on0) sx[c0] = xb0;
    if (on1) sx[c1] = xb1;
    ff_wave_sync();
    ff_wave_forces(t, sx, sf, stage, lane, e);
    const double eb = ((e[0] + e[1]) + e[2]) + e[3];
    // the Metropolis rule: the same bits in every lane
    const double ta = (double)p.T[ra], tb = (double)p.T[rb];
    const double beta_a = 1.0 / (TI_FF_GAS_CONSTANT * ta), beta_b = 1.0 / (TI_FF_GAS_CONSTANT * tb);
    const double delta = (beta_a - beta_b) * (ea - eb);
    const long long id = p.ladder_ids ? p.ladder_ids[l] : l;
    uint32_t c[4] = {(uint32_t)id, (uint32_t)((uint64_t)id >> 32), (uint32_t)p.attempt, TI_REMD_DOMAIN + (uint32_t)(k >> 2)};
    philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    const double logu = (double)vl_host_logf(vl_uniform24(c[k & 3]));
    const bool accept = isfinite(ea) && isfinite(eb) && p.flag[ra] == 0 && p.flag[rb] == 0 && (delta >= 0.0 || logu < delta);
    if (accept) {
        // The Langevin kernel stores the velocity half a kick behind the positions: v = w - (dt / 2) f(x) / m, w the velocity at x.
        // It is w that is Maxwell-distributed and independent of x, so it is w that is rescaled: the configuration that moves to a
        // row takes (w sqrt(T_new / T_old)) - (dt / 2) f(x) / m with it, its own half kick h added and taken off again.
        const double up = sqrt(tb / ta), down = sqrt(ta / tb);          // row k + 1 receives w(k) up, row k receives w(k + 1) down
        if (on0) {
            const double va = p.vel[ra * m3 + c0], vb = p.vel[rb * m3 + c0], hb0 = half * sf[c0] / m0;
            p.pos[ra * m3 + c0] = xb0; p.pos[rb * m3 + c0] = xa0;
            p.vel[ra * m3 + c0] = (vb + hb0) * down - hb0; p.vel[rb * m3 + c0] = (va + ha0) * up - ha0;
        }
        if (on1) {
            const double va = p.vel[ra * m3 + c1], vb = p.vel[rb * m3 + c1], hb1 = half * sf[c1] / m1;
            p.pos[ra * m3 + c1] = xb1; p.pos[rb * m3 + c1] = xa1;
            p.vel[ra * m3 + c1] = (vb + hb1) * down - hb1; p.vel[rb * m3 + c1] = (va + ha1) * up - ha1;
        }
    }
    if (lane == 0) {
        int32_t wa = p.walker[ra], wb = p.walker[rb];
        if (accept) {
            p.walker[ra] = wb; p.walker[rb] = wa;
            const int32_t s = wa; wa = wb; wb = s;
        }
        if (p.out_walker) { p.out_walker[ra] = wa; p.out_walker[rb] = wb; }
        if (p.counts) {
            long long* cnt = p.counts + (l * (K - 1) + k) * 2;
            cnt[0] = cnt[0] + 1;
            if (accept) cnt[1] = cnt[1] + 1;
        }
    }
}

// one workgroup walks the labels grid-stride; the smallest bad index by the block tree, as obs_ff_bad_temperature_kernel finds its own
constexpr int REMD_WALKER_BLOCK = 256;
__global__ __launch_bounds__(REMD_WALKER_BLOCK) void obs_ff_remd_walker_kernel(int32_t* __restrict__ work, const int32_t* __restrict__ in,
                                                                              long long B, int K, double* __restrict__ bad_out)
{
    __shared__ double sm[REMD_WALKER_BLOCK];
    double bad = HUGE_VAL;
    for (long long i = threadIdx.x; i < B; i += REMD_WALKER_BLOCK) {
        const int32_t v = in ? in[i] : (int32_t)(i % K);
        if (v < 0 || v >= K) bad = fmin(bad, (double)i);
        work[i] = v;
    }
    sm[threadIdx.x] = bad;
    __syncthreads();
    for (int s = REMD_WALKER_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmin(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && sm[0] < (double)B && !(bad_out[0] < (double)B)) bad_out[0] = -1.0 - sm[0];
}

}  // namespace

hipError_t launch_obs_ff_remd(const RemdParams& p, hipStream_t st)
{
    if (p.B < 1 || p.K < 2) return hipSuccess;
    const long long pairs = (p.K - (int)(p.attempt & 1)) / 2, waves = (p.B / p.K) * (pairs > 0 ? pairs : 1);
    hipLaunchKernelGGL(obs_ff_remd_kernel, dim3((unsigned)((waves + FF_WAVES - 1) / FF_WAVES)), dim3(64 * FF_WAVES), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_obs_ff_remd_walker(int32_t* work, const int32_t* in, long long B, int K, double* bad, hipStream_t st)
{
    hipLaunchKernelGGL(obs_ff_remd_walker_kernel, dim3(1), dim3(REMD_WALKER_BLOCK), 0, st, work, in, B, K, bad);
    return hipGetLastError();
}

}  // namespace ti
