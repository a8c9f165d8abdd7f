// obs_ff_md_kernels.hip -- force-field forces (include/ti_hip.h ti_obs_ff_forces) and Langevin dynamics with them (ti_obs_ff_langevin).
// Both kernels run one wave per molecule / replica, FF_WAVES per workgroup, stage the tables in LDS once per workgroup and evaluate
// the forces through ff_wave_forces (ff_device.hpp): the integrator runs the code the forces entry point pins.  fp64 throughout, no
// contraction, no atomics; a molecule's outputs do not depend on its wave, workgroup, trip or place in the batch.
//
// The Langevin kernel keeps a replica's positions, velocities and forces in LDS for the whole launch.  After the tables are staged
// there is no workgroup barrier: the waves of a workgroup advance independently, and a replica whose state turns non-finite leaves
// the loop alone.  Step s (global index step0 + s) of OpenMM's "middle" scheme:
//   v += dt f(x) / m;  x += (dt / 2) v;  v = a v + sqrt((1 - a^2) R T / m) xi;  x += (dt / 2) v
// xi[a][c] = the Philox normal (seed, id, step0 + s, 3a + c) of vloss_normal.hpp promoted to fp64; a == 1 (no friction): no draw.
// The forces are evaluated once per step, at the top of the loop, from the positions the previous step (or the previous launch) left:
// one call site, so a call cut into launches repeats the uncut call bit for bit.
#include "ff_device.hpp"
#include "ff_stage.hpp"
#include "adw_device.hpp"
#include "vloss_normal.hpp"

namespace ti {

namespace {

__global__ __launch_bounds__(64 * FF_WAVES) void obs_ff_forces_kernel(FfForceParams p)
{
#pragma clang fp contract(off)
    __shared__ int32_t s_idx[FFD_IDX_WORDS];
    __shared__ double s_par[FFD_PAR_DOUBLES];
    __shared__ int32_t s_inc[FF_INC_WORDS];
    __shared__ double s_x[FF_WAVES][FFD_X_DOUBLES], s_f[FF_WAVES][FFD_X_DOUBLES], s_stage[FF_WAVES][FF_STAGE_DOUBLES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const FfView t = ff_stage_tables(p.t, s_idx, s_par, s_inc);
    double *sx = s_x[wave], *sf = s_f[wave];
    const int m3 = 3 * t.A;
    __syncthreads();                                        // the tables
    for (long long base = (long long)blockIdx.x * FF_WAVES; base < p.B; base += (long long)gridDim.x * FF_WAVES) {
        const long long b = base + wave;
        if (b >= p.B) continue;                             // no workgroup barrier below: a wave past the end just idles
        for (int c = lane; c < m3; c += 64) sx[c] = (double)p.x[b * m3 + c] * p.to_nm;
        ff_wave_sync();
        double e[4];
        ff_wave_forces(t, sx, sf, s_stage[wave], lane, e);
        double rt = 1.0;
        if (p.T) rt = TI_FF_GAS_CONSTANT * (double)p.T[b];
        for (int c = lane; c < m3; c += 64) p.f[b * m3 + c] = p.T ? sf[c] / rt : sf[c];
        if (p.e && lane == 0) {
            if (p.T) { e[0] = e[0] / rt; e[1] = e[1] / rt; e[2] = e[2] / rt; e[3] = e[3] / rt; }
            p.e[b] = ((e[0] + e[1]) + e[2]) + e[3];
        }
        ff_wave_sync();                                     // the next trip overwrites sx and sf
    }
}

// the Philox normal of (seed, replica, step, component) as vloss_kernels.hip draws z and oracle.normal returns it
__device__ __forceinline__ double md_normal(uint64_t seed, long long traj, long long step, int comp)
{
    uint32_t c[4] = {(uint32_t)traj, (uint32_t)((uint64_t)traj >> 32), (uint32_t)step, (uint32_t)(comp >> 2)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int pair = (comp & 3) >> 1;
    return (double)vl_box_muller(c[2 * pair], c[2 * pair + 1], comp & 1);
}

__global__ __launch_bounds__(64 * FF_WAVES) void obs_ff_langevin_kernel(MdParams p)
{
#pragma clang fp contract(off)
    __shared__ int32_t s_idx[FFD_IDX_WORDS];
    __shared__ double s_par[FFD_PAR_DOUBLES];
    __shared__ int32_t s_inc[FF_INC_WORDS];
    __shared__ double s_mass[FF_MAX_ATOMS];
    __shared__ double s_x[FF_WAVES][FFD_X_DOUBLES], s_v[FF_WAVES][FFD_X_DOUBLES], s_f[FF_WAVES][FFD_X_DOUBLES];
    __shared__ double s_stage[FF_WAVES][FF_STAGE_DOUBLES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const FfView t = ff_stage_tables(p.t, s_idx, s_par, s_inc);
    if ((int)threadIdx.x < t.A) s_mass[threadIdx.x] = p.mass[threadIdx.x];
    __syncthreads();                                        // the only workgroup barrier: tables and masses
    const long long b = (long long)blockIdx.x * FF_WAVES + wave;
    if (p.bad_T[0] < (double)p.B) return;                   // a refused temperature: the host reports it, nothing is written
    if (b >= p.B || p.flag[b] != 0) return;                 // past the end, or stopped in an earlier launch
    double *sx = s_x[wave], *sv = s_v[wave], *sf = s_f[wave], *stage = s_stage[wave];
    const int A = t.A, m3 = 3 * A;
    const long long id = p.ids ? p.ids[b] : p.traj_offset + b;
    const double rt = TI_FF_GAS_CONSTANT * (double)p.T[b];
    // this lane's components c0 = lane and c1 = lane + 64 (3A <= 75), their masses and noise amplitudes
    const int c0 = lane, c1 = lane + 64;
    const bool on0 = c0 < m3, on1 = c1 < m3;
    const double m0 = on0 ? s_mass[c0 / 3] : 1.0, m1 = on1 ? s_mass[c1 / 3] : 1.0;
    const double amp0 = sqrt((1.0 - p.a * p.a) * rt / m0), amp1 = sqrt((1.0 - p.a * p.a) * rt / m1);
    const double half = p.dt * 0.5;
    if (on0) sx[c0] = p.pos[b * m3 + c0];
    if (on1) sx[c1] = p.pos[b * m3 + c1];
    if (p.draw) {                                           // N(0, R T / m): components 3A + c at the first step's index
        if (on0) sv[c0] = sqrt(rt / m0) * md_normal(p.seed, id, p.step0, m3 + c0);
        if (on1) sv[c1] = sqrt(rt / m1) * md_normal(p.seed, id, p.step0, m3 + c1);
    } else {
        if (on0) sv[c0] = p.vel[b * m3 + c0];
        if (on1) sv[c1] = p.vel[b * m3 + c1];
    }
    ff_wave_sync();
    bool dead = false;
    for (long long s = 0;; ++s) {
        double e[4];
        ff_wave_forces(t, sx, sf, stage, lane, e);          // the forces at the positions of the step before (or of the launch's start)
        const long long done = p.steps_before + s;          // steps of the call behind the state
        if (s > 0 && p.stride > 0 && done % p.stride == 0) {
            const long long row = b * p.n_frames + (done / p.stride - 1);
            if (p.frames) {
                if (lane < 3) {                             // the unweighted mean: the atoms in order
                    double mean = 0.0;
                    for (int k = 0; k < A; ++k) mean = mean + sx[3 * k + lane];
                    stage[lane] = mean / (double)A;
                }
                ff_wave_sync();
                if (on0) p.frames[row * m3 + c0] = (float)((sx[c0] - stage[c0 % 3]) / p.to_nm);
                if (on1) p.frames[row * m3 + c1] = (float)((sx[c1] - stage[c1 % 3]) / p.to_nm);
                ff_wave_sync();                             // the next force evaluation writes the staging area
            }
            if (p.epot && lane == 0) p.epot[row] = ((e[0] + e[1]) + e[2]) + e[3];
            if (p.ekin) {
                double k2 = (on0 ? m0 * sv[c0] * sv[c0] * 0.5 : 0.0) + (on1 ? m1 * sv[c1] * sv[c1] * 0.5 : 0.0);
                k2 = wave_sum(k2);
                if (lane == 0) p.ekin[row] = k2;
            }
        }
        if (s == p.n_steps) break;
        const long long step = p.step0 + s;
        bool bad = false;
        if (on0) {
            double v = sv[c0] + p.dt * sf[c0] / m0, x = sx[c0] + half * v;
            if (p.a != 1.0) v = p.a * v + amp0 * md_normal(p.seed, id, step, c0);
            x = x + half * v;
            sv[c0] = v; sx[c0] = x;
            bad = !(isfinite(v) && isfinite(x));
        }
        if (on1) {
            double v = sv[c1] + p.dt * sf[c1] / m1, x = sx[c1] + half * v;
            if (p.a != 1.0) v = p.a * v + amp1 * md_normal(p.seed, id, step, c1);
            x = x + half * v;
            sv[c1] = v; sx[c1] = x;
            bad = bad || !(isfinite(v) && isfinite(x));
        }
        ff_wave_sync();
        if (__any(bad)) { dead = true; break; }
    }
    if (dead) {
        if (lane == 0) p.flag[b] = 1 + p.launch;            // an ordinary store; the state of a stopped replica is not written back
        return;
    }
    if (on0) { p.pos[b * m3 + c0] = sx[c0]; p.vel[b * m3 + c0] = sv[c0]; }
    if (on1) { p.pos[b * m3 + c1] = sx[c1]; p.vel[b * m3 + c1] = sv[c1]; }
}

}  // namespace

hipError_t launch_obs_ff_forces(const FfForceParams& p, hipStream_t st)
{
    if (p.B < 1) return hipSuccess;
    const long long groups = std::min<long long>((p.B + FF_WAVES - 1) / FF_WAVES, 4096);
    hipLaunchKernelGGL(obs_ff_forces_kernel, dim3((unsigned)groups), dim3(64 * FF_WAVES), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_obs_ff_langevin(const MdParams& p, hipStream_t st)
{
    if (p.B < 1) return hipSuccess;
    hipLaunchKernelGGL(obs_ff_langevin_kernel, dim3((unsigned)((p.B + FF_WAVES - 1) / FF_WAVES)), dim3(64 * FF_WAVES), 0, st, p);
    return hipGetLastError();
}

}  // namespace ti
