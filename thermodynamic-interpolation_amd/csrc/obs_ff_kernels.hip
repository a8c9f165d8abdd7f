// obs_ff_kernels.hip -- force-field energies (include/ti_hip.h ti_obs_ff_energy, ti_obs_ti_logw): the harmonic bond, harmonic angle,
// periodic torsion and non-bonded (Lennard-Jones + Coulomb, no cutoff) sums of every molecule of a batch, in fp64 from the fp32
// coordinates.  One wave per molecule, FF_WAVES molecules per workgroup.  A workgroup stages the term words and parameters in LDS
// once and then walks its molecules; a molecule's positions go to LDS as fp64 nm.  Lane l adds terms l, l + 64, ... of a table in
// that order and the 64 lane sums are combined by the fixed butterfly of wave_sum, so a molecule's result is a function of its
// coordinates, to_nm, T_b and the tables only: which wave, which workgroup and which trip computes it does not enter.  No atomics.
#include "ode_device.hpp"

namespace ti {

namespace {

constexpr int FF_IDX_WORDS = TI_FF_MAX_BONDS + TI_FF_MAX_ANGLES + TI_FF_MAX_TORSIONS + TI_FF_MAX_PAIRS;
constexpr int FF_PAR_DOUBLES = 2 * TI_FF_MAX_BONDS + 2 * TI_FF_MAX_ANGLES + 2 * TI_FF_MAX_TORSIONS + 3 * TI_FF_MAX_PAIRS;
constexpr int FF_X_DOUBLES = 3 * FF_MAX_ATOMS + 1;

struct P3 { double x, y, z; };
__device__ __forceinline__ P3 at(const double* __restrict__ s, int a) { return P3{s[3 * a], s[3 * a + 1], s[3 * a + 2]}; }
__device__ __forceinline__ P3 sub3(P3 a, P3 b) { return P3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(P3 a, P3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ P3 cross3(P3 a, P3 b) { return P3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

__global__ __launch_bounds__(64 * FF_WAVES) void obs_ff_energy_kernel(FfParams p)
{
    __shared__ int32_t s_idx[FF_IDX_WORDS];
    __shared__ double s_par[FF_PAR_DOUBLES];
    __shared__ double s_x[FF_WAVES][FF_X_DOUBLES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_idx = p.nb + p.na + p.nt + p.np, n_par = 2 * (p.nb + p.na + p.nt) + 3 * p.np;
    for (int i = threadIdx.x; i < n_idx; i += 64 * FF_WAVES) s_idx[i] = p.idx[i];
    for (int i = threadIdx.x; i < n_par; i += 64 * FF_WAVES) s_par[i] = p.par[i];
    const int32_t *wb = s_idx, *wa = wb + p.nb, *wt = wa + p.na, *wp = wt + p.nt;
    const double *pb = s_par, *pa = pb + 2 * p.nb, *pt = pa + 2 * p.na, *pp = pt + 2 * p.nt;
    double* sx = s_x[wave];
    const int m3 = 3 * p.A;
    // every wave of the workgroup takes the same number of trips (the barriers are uniform); a wave past the end of the batch idles
    for (long long base = (long long)blockIdx.x * FF_WAVES; base < p.B; base += (long long)gridDim.x * FF_WAVES) {
        const long long b = base + wave;
        const bool on = b < p.B;
        __syncthreads();                                    // the tables (first trip); the previous trip's reads of sx
        if (on)
            for (int c = lane; c < m3; c += 64) sx[c] = (double)p.x[b * m3 + c] * p.to_nm;
        __syncthreads();
        if (!on) continue;
        double eb = 0.0, ea = 0.0, et = 0.0, ep = 0.0;
        for (int t = lane; t < p.nb; t += 64) {             // k (r - r0)^2 / 2
            const int32_t w = wb[t];
            const P3 d = sub3(at(sx, ff_atom(w, 1)), at(sx, ff_atom(w, 0)));
            const double dr = sqrt(dot3(d, d)) - pb[2 * t];
            eb += pb[2 * t + 1] * dr * dr * 0.5;
        }
        for (int t = lane; t < p.na; t += 64) {             // k (theta - theta0)^2 / 2, theta at j
            const int32_t w = wa[t];
            const P3 c = at(sx, ff_atom(w, 1)), u = sub3(at(sx, ff_atom(w, 0)), c), v = sub3(at(sx, ff_atom(w, 2)), c);
            double cs = dot3(u, v) / (sqrt(dot3(u, u)) * sqrt(dot3(v, v)));
            cs = cs > 1.0 ? 1.0 : cs < -1.0 ? -1.0 : cs;    // a NaN stays a NaN
            const double dth = acos(cs) - pa[2 * t];
            ea += pa[2 * t + 1] * dth * dth * 0.5;
        }
        for (int t = lane; t < p.nt; t += 64) {             // k (1 + cos(n phi - phase))
            const int32_t w = wt[t];
            const P3 x1 = at(sx, ff_atom(w, 0)), x2 = at(sx, ff_atom(w, 1)), x3 = at(sx, ff_atom(w, 2)), x4 = at(sx, ff_atom(w, 3));
            const P3 b1 = sub3(x2, x1), b2 = sub3(x3, x2), b3 = sub3(x4, x3), c23 = cross3(b2, b3);
            const double phi = atan2(sqrt(dot3(b2, b2)) * dot3(b1, c23), dot3(cross3(b1, b2), c23));
            et += pt[2 * t + 1] * (1.0 + cos((double)ff_period(w) * phi - pt[2 * t]));
        }
        for (int t = lane; t < p.np; t += 64) {             // 4 eps s (s - 1) + coulomb qq / r, s = (sigma / r)^6
            const int32_t w = wp[t];
            if (!(w & FF_LIVE)) continue;
            const P3 d = sub3(at(sx, ff_atom(w, 1)), at(sx, ff_atom(w, 0)));
            const double r = sqrt(dot3(d, d)), qq = pp[3 * t], sigma = pp[3 * t + 1], eps = pp[3 * t + 2];
            double lj = 0.0, cl = 0.0;
            if (eps > 0.0 && sigma > 0.0) {
                const double q = sigma / r, q2 = q * q, s6 = q2 * q2 * q2;
                lj = 4.0 * eps * s6 * (s6 - 1.0);
            }
            if (qq != 0.0) cl = p.coulomb * qq / r;
            ep += (lj == HUGE_VAL) ? lj : lj + cl;          // r = 0: the wall wins over an attractive charge product
        }
        eb = wave_sum(eb); ea = wave_sum(ea); et = wave_sum(et); ep = wave_sum(ep);
        if (lane == 0) {
            if (p.T) {
                const double rt = TI_FF_GAS_CONSTANT * (double)p.T[b];
                eb /= rt; ea /= rt; et /= rt; ep /= rt;
            }
            p.e[b] = ((eb + ea) + et) + ep;
            if (p.terms) { p.terms[4 * b] = eb; p.terms[4 * b + 1] = ea; p.terms[4 * b + 2] = et; p.terms[4 * b + 3] = ep; }
        }
    }
}

// one workgroup walks T grid-stride; the smallest bad index by the block tree (min is order-independent)
__global__ __launch_bounds__(RED_BLOCK) void obs_ff_bad_temperature_kernel(double* __restrict__ out, const float* __restrict__ T, long long B)
{
    __shared__ double sm[RED_BLOCK];
    double bad = HUGE_VAL;
    for (long long i = threadIdx.x; i < B; i += RED_BLOCK) {
        const float v = T[i];
        if (!(isfinite(v) && v > 0.f)) bad = fmin(bad, (double)i);
    }
    sm[threadIdx.x] = bad;
    __syncthreads();
    for (int s = RED_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmin(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sm[0];
}

__global__ __launch_bounds__(256) void obs_ti_logw_kernel(float* __restrict__ logw, const double* __restrict__ u0, const double* __restrict__ u1,
                                                         const float* __restrict__ neg_dlogp, long long B)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const double a = u0 ? u0[i] : 0.0, n = neg_dlogp ? (double)neg_dlogp[i] : 0.0;
    logw[i] = (float)-((u1[i] - a) + n);
}

}  // namespace

hipError_t launch_obs_ff_energy(const FfParams& p, hipStream_t st)
{
    if (p.B < 1) return hipSuccess;
    // enough workgroups to fill the chip several times over at the product's batches; the result does not depend on the cut
    const long long groups = std::min<long long>((p.B + FF_WAVES - 1) / FF_WAVES, 4096);
    hipLaunchKernelGGL(obs_ff_energy_kernel, dim3((unsigned)groups), dim3(64 * FF_WAVES), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_obs_ff_bad_temperature(double* out, const float* T, long long B, hipStream_t st)
{
    hipLaunchKernelGGL(obs_ff_bad_temperature_kernel, dim3(1), dim3(RED_BLOCK), 0, st, out, T, B);
    return hipGetLastError();
}

hipError_t launch_obs_ti_logw(float* logw, const double* u0, const double* u1, const float* neg_dlogp, long long B, hipStream_t st)
{
    if (B > 0) hipLaunchKernelGGL(obs_ti_logw_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, logw, u0, u1, neg_dlogp, B);
    return hipGetLastError();
}

}  // namespace ti
