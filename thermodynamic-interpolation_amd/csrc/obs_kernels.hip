// obs_kernels.hip -- observables (include/ti_hip.h ti_obs_*): per-molecule collective variables, importance weights and weighted
// histograms, computed where the coordinates live.  Arithmetic is fp64 on fp32 inputs.  No atomics feed any result: per-molecule
// values are computed by one thread in atom order (they do not depend on the rest of the batch), batch-wide sums are per-block
// partials in a fixed tree order (ode_device.hpp) combined block by block by a second kernel, so a result is a function of the
// inputs and the launch shape (B -> obs_blocks(B) blocks of 256 threads) only and repeats bit for bit.
#include "ode_device.hpp"

namespace ti {

namespace {

// ---- collective variables ------------------------------------------------------------------------------------------------------
// Largest eigenvalue of the symmetric 4x4 matrix `a` by cyclic Jacobi rotations, a fixed number of sweeps (the off-diagonal norm
// falls quadratically; 4x4 matrices are at round-off after 5-6 sweeps).  Every index is a compile-time constant, so `a` lives in
// registers.  Rank-deficient input (zero, rank-1, ... matrices) needs no special case: a zero pivot is skipped.
constexpr int JACOBI_SWEEPS = 10;

__device__ __forceinline__ double jacobi_max_eig4(double (&a)[4][4])
{
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq != 0.0) {
                    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                    // tan of the rotation angle, the smaller root; |theta| huge: theta^2 = inf, t = 0 (the pivot is below round-off)
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (r != p && r != q) {
                            const double arp = a[r][p], arq = a[r][q];
                            a[r][p] = a[p][r] = c * arp - s * arq;
                            a[r][q] = a[q][r] = s * arp + c * arq;
                        }
                    }
                    a[p][p] -= t * apq;
                    a[q][q] += t * apq;
                    a[p][q] = a[q][p] = 0.0;
                }
            }
        }
    }
    return fmax(fmax(a[0][0], a[1][1]), fmax(a[2][2], a[3][3]));
}

// Minimal RMSD over proper rotations of the selected atoms a < n of xb to ref, both centred over those atoms (Horn 1987: the
// largest eigenvalue lambda of the 4x4 quaternion matrix of the covariance S is max_R sum_a (R x_a) . r_a over rotations R, so
// rmsd^2 = (|x|^2 + |r|^2 - 2 lambda) / count; reflections are not among the R, a mirror image does not give 0).
__device__ double rmsd_of(const float* __restrict__ xb, const float* __restrict__ ref, const int32_t* __restrict__ sel, int n)
{
    double cx = 0, cy = 0, cz = 0, rx = 0, ry = 0, rz = 0;
    int cnt = 0;
    for (int a = 0; a < n; ++a) {
        if (sel && !sel[a]) continue;
        cx += (double)xb[3 * a]; cy += (double)xb[3 * a + 1]; cz += (double)xb[3 * a + 2];
        rx += (double)ref[3 * a]; ry += (double)ref[3 * a + 1]; rz += (double)ref[3 * a + 2];
        ++cnt;
    }
    if (cnt == 0) return __longlong_as_double(0x7ff8000000000000LL);
    const double inv = 1.0 / (double)cnt;
    cx *= inv; cy *= inv; cz *= inv; rx *= inv; ry *= inv; rz *= inv;
    double sxx = 0, sxy = 0, sxz = 0, syx = 0, syy = 0, syz = 0, szx = 0, szy = 0, szz = 0, e0 = 0;
    for (int a = 0; a < n; ++a) {
        if (sel && !sel[a]) continue;
        const double px = (double)xb[3 * a] - cx, py = (double)xb[3 * a + 1] - cy, pz = (double)xb[3 * a + 2] - cz;
        const double qx = (double)ref[3 * a] - rx, qy = (double)ref[3 * a + 1] - ry, qz = (double)ref[3 * a + 2] - rz;
        e0 += px * px + py * py + pz * pz + qx * qx + qy * qy + qz * qz;
        sxx += px * qx; sxy += px * qy; sxz += px * qz;
        syx += py * qx; syy += py * qy; syz += py * qz;
        szx += pz * qx; szy += pz * qy; szz += pz * qz;
    }
    double m[4][4];
    m[0][0] = sxx + syy + szz; m[1][1] = sxx - syy - szz; m[2][2] = -sxx + syy - szz; m[3][3] = -sxx - syy + szz;
    m[0][1] = m[1][0] = syz - szy; m[0][2] = m[2][0] = szx - sxz; m[0][3] = m[3][0] = sxy - syx;
    m[1][2] = m[2][1] = sxy + syx; m[1][3] = m[3][1] = szx + sxz; m[2][3] = m[3][2] = syz + szy;
    const double lambda = jacobi_max_eig4(m);
    return sqrt(fmax(e0 - 2.0 * lambda, 0.0) * inv);
}

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 atom(const float* __restrict__ xb, int a) { return V3{(double)xb[3 * a], (double)xb[3 * a + 1], (double)xb[3 * a + 2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// One thread per (molecule, descriptor).  desc [K][5] = (kind, i, j, k, l).
__global__ __launch_bounds__(256) void obs_cv_kernel(ObsCvParams p)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.B * p.K) return;
    const long long b = idx / p.K;
    const int32_t* __restrict__ d = p.desc + 5 * (int)(idx - b * p.K);
    const float* __restrict__ xb = p.x + b * p.m;
    const int kind = d[0];
    const int n = p.n_atoms ? p.n_atoms[b] : p.A;           // real atoms of this molecule; pads are never read
    double out;
    if (kind == TI_OBS_COORD) {
        out = (double)xb[d[1]];
    } else if (kind == TI_OBS_RMSD) {
        out = rmsd_of(xb, p.ref, p.sel, n);
    } else {
        const int na = kind == TI_OBS_DIST ? 2 : kind == TI_OBS_ANGLE ? 3 : 4;
        bool pad = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) pad = pad || (j < na && d[1 + j] >= n);
        if (pad) {
            out = __longlong_as_double(0x7ff8000000000000LL);
        } else if (kind == TI_OBS_DIST) {                    // |x_j - x_i|
            const V3 r = sub(atom(xb, d[2]), atom(xb, d[1]));
            out = sqrt(dot(r, r));
        } else if (kind == TI_OBS_ANGLE) {                   // angle at j between j->i and j->k, [0, pi]
            const V3 c = atom(xb, d[2]), u = sub(atom(xb, d[1]), c), v = sub(atom(xb, d[3]), c), w = cross(u, v);
            out = atan2(sqrt(dot(w, w)), dot(u, v));
        } else {                                             // atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3)), (-pi, pi]
            const V3 x1 = atom(xb, d[1]), x2 = atom(xb, d[2]), x3 = atom(xb, d[3]), x4 = atom(xb, d[4]);
            const V3 b1 = sub(x2, x1), b2 = sub(x3, x2), b3 = sub(x4, x3), c23 = cross(b2, b3);
            out = atan2(sqrt(dot(b2, b2)) * dot(b1, c23), dot(cross(b1, b2), c23));
        }
    }
    p.cv[idx] = (float)out;
}

// ---- importance weights and histograms -----------------------------------------------------------------------------------------
constexpr int OBS_WAVES = RED_BLOCK / 64;

// block reduction in the fixed tree order of block_sum; op 0 sum, 1 max, 2 min.  Result in every thread; safe to call repeatedly.
__device__ __forceinline__ double block_reduce(double v, int op)
{
    __shared__ double sm[RED_BLOCK];
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = RED_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double a = sm[threadIdx.x], b = sm[threadIdx.x + s];
            sm[threadIdx.x] = op == 0 ? a + b : op == 1 ? fmax(a, b) : fmin(a, b);
        }
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// partial [blocks][2]: the largest finite logw of the block's entries (-inf: none) and the smallest index of a non-finite entry as a
// double (+inf: none; indices are exact in fp64)
__global__ __launch_bounds__(RED_BLOCK) void obs_logw_max_kernel(double* __restrict__ partial, const float* __restrict__ logw, long long B)
{
    double mx = -HUGE_VAL, bad = HUGE_VAL;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < B; i += (long long)gridDim.x * RED_BLOCK) {
        const float v = logw[i];
        if (isfinite(v)) mx = fmax(mx, (double)v);
        else bad = fmin(bad, (double)i);
    }
    mx = block_reduce(mx, 1);
    bad = block_reduce(bad, 2);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = mx; partial[2 * blockIdx.x + 1] = bad; }
}

// partial [blocks][2]: sum w and sum w^2 with w = exp(logw - max), each thread's entries in index order, then the block tree
__global__ __launch_bounds__(RED_BLOCK) void obs_logw_kernel(double* __restrict__ partial, const float* __restrict__ logw, const double* __restrict__ mx,
                                                            long long B)
{
    const double m = *mx;
    double s1 = 0.0, s2 = 0.0;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < B; i += (long long)gridDim.x * RED_BLOCK) {
        const double w = exp((double)logw[i] - m);
        s1 += w; s2 += w * w;
    }
    s1 = block_reduce(s1, 0);
    s2 = block_reduce(s2, 0);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = s1; partial[2 * blockIdx.x + 1] = s2; }
}

// out[c] = partial[0][c] op partial[1][c] op ... in block order; op of column c: bits 2c, 2c+1 of `ops` for c < 16 (0 sum, 1 max, 2 min), sum beyond
__global__ __launch_bounds__(RED_BLOCK) void obs_combine_kernel(double* __restrict__ out, const double* __restrict__ partial, int nb, int ncol, unsigned ops)
{
    const int c = blockIdx.x * RED_BLOCK + threadIdx.x;
    if (c >= ncol) return;
    const int op = c < 16 ? (ops >> (2 * c)) & 3 : 0;
    double acc = partial[c];
    for (int k = 1; k < nb; ++k) {
        const double v = partial[(size_t)k * ncol + c];
        acc = op == 0 ? acc + v : op == 1 ? fmax(acc, v) : fmin(acc, v);
    }
    out[c] = acc;
}

// norm = (max, sum w): w_i = exp(logw_i - max) / sum w as fp32
__global__ __launch_bounds__(256) void obs_weights_kernel(float* __restrict__ w, const float* __restrict__ logw, const double* __restrict__ norm, long long B)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < B) w[i] = (float)(exp((double)logw[i] - norm[0]) / norm[1]);
}

// bin of v among n_bins equal bins on [lo, hi) with edges e_k = lo + ((hi - lo) k) / n_bins: e_k <= v < e_k+1 (a value on an interior
// edge goes up); n_bins: below lo, n_bins + 1: hi and above, n_bins + 2: not finite.  The estimate is off by one at most; the
// comparisons with the edges decide.
__device__ __forceinline__ int bin_of(float vf, int n_bins, double lo, double hi)
{
    if (!isfinite(vf)) return n_bins + 2;
    const double v = (double)vf, span = hi - lo;
    if (v < lo) return n_bins;
    if (v >= hi) return n_bins + 1;
    int k = (int)floor((v - lo) * (double)n_bins / span);
    k = k < 0 ? 0 : k > n_bins - 1 ? n_bins - 1 : k;
    if (v < lo + (span * (double)k) / (double)n_bins) --k;
    else if (k + 1 < n_bins && v >= lo + (span * (double)(k + 1)) / (double)n_bins) ++k;
    return k < 0 ? 0 : k;
}

constexpr int OBS_BIN_CHUNKS = 5;          // 256 bins + 3 tails <= 5 x 64 accumulators, bin c * 64 + j in lane j's acc[c]

// partial [blocks][n_bins + 3]: weighted counts of the block's values.  A wave takes 64 values per trip; for every bin present among
// them the fixed-tree wave sum of (bin == b ? w : 0) is added to the accumulator of the lane that owns b -- one add per bin and trip,
// so the order in which the bins of a trip are visited does not matter; trips follow in index order.  The four waves of a block are
// then added in wave order.  norm = (max, sum w) of logw, or logw == NULL: every weight is 1 / B.
__global__ __launch_bounds__(RED_BLOCK) void obs_whist_kernel(double* __restrict__ partial, const float* __restrict__ values, long long stride,
                                                             const float* __restrict__ logw, const double* __restrict__ norm, long long B, int n_bins,
                                                             double lo, double hi)
{
    __shared__ double sm[OBS_WAVES][OBS_BIN_CHUNKS * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nb = n_bins + 3;
    const double m = logw ? norm[0] : 0.0, tot = logw ? norm[1] : (double)B;
    double acc[OBS_BIN_CHUNKS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long base = ((long long)blockIdx.x * OBS_WAVES + wave) * 64; base < B; base += (long long)gridDim.x * RED_BLOCK) {
        const long long i = base + lane;
        int bin = -1;
        double w = 0.0;
        if (i < B) {
            bin = bin_of(values[i * stride], n_bins, lo, hi);
            w = (logw ? exp((double)logw[i] - m) : 1.0) / tot;
        }
        unsigned long long pending = __ballot(bin >= 0);
        while (pending) {                                     // wave-uniform
            const int bb = __shfl(bin, __ffsll((long long)pending) - 1);
            const bool mine = bin == bb;
            const double s = wave_sum(mine ? w : 0.0);
#pragma unroll
            for (int c = 0; c < OBS_BIN_CHUNKS; ++c)
                if (c == (bb >> 6) && lane == (bb & 63)) acc[c] += s;
            pending &= ~__ballot(mine);
        }
    }
#pragma unroll
    for (int c = 0; c < OBS_BIN_CHUNKS; ++c) sm[wave][c * 64 + lane] = acc[c];
    __syncthreads();
    for (int c = threadIdx.x; c < nb; c += RED_BLOCK) {
        double t = sm[0][c];
#pragma unroll
        for (int w2 = 1; w2 < OBS_WAVES; ++w2) t += sm[w2][c];
        partial[(size_t)blockIdx.x * nb + c] = t;
    }
}

}  // namespace

int obs_blocks(long long B) { return (int)std::min<long long>(OBS_MAX_BLOCKS, std::max<long long>(1, (B + RED_BLOCK - 1) / RED_BLOCK)); }

hipError_t launch_obs_cv(const ObsCvParams& p, hipStream_t st)
{
    const long long n = p.B * p.K;
    if (n > 0) hipLaunchKernelGGL(obs_cv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_obs_logw_max(double* out, double* partial, const float* logw, long long B, hipStream_t st)
{
    const int nb = obs_blocks(B);
    hipLaunchKernelGGL(obs_logw_max_kernel, dim3(nb), dim3(RED_BLOCK), 0, st, partial, logw, B);
    hipLaunchKernelGGL(obs_combine_kernel, dim3(1), dim3(RED_BLOCK), 0, st, out, partial, nb, 2, 1u | (2u << 2));
    return hipGetLastError();
}

hipError_t launch_obs_logw_sums(double* out, double* partial, const float* logw, const double* mx, long long B, hipStream_t st)
{
    const int nb = obs_blocks(B);
    hipLaunchKernelGGL(obs_logw_kernel, dim3(nb), dim3(RED_BLOCK), 0, st, partial, logw, mx, B);
    hipLaunchKernelGGL(obs_combine_kernel, dim3(1), dim3(RED_BLOCK), 0, st, out, partial, nb, 2, 0u);
    return hipGetLastError();
}

hipError_t launch_obs_weights(float* w, const float* logw, const double* norm, long long B, hipStream_t st)
{
    if (B > 0) hipLaunchKernelGGL(obs_weights_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, w, logw, norm, B);
    return hipGetLastError();
}

hipError_t launch_obs_whist(double* out, double* partial, const float* values, long long stride, const float* logw, const double* norm, long long B,
                            int n_bins, double lo, double hi, hipStream_t st)
{
    const int nb = obs_blocks(B), ncol = n_bins + 3;
    hipLaunchKernelGGL(obs_whist_kernel, dim3(nb), dim3(RED_BLOCK), 0, st, partial, values, stride, logw, norm, B, n_bins, lo, hi);
    hipLaunchKernelGGL(obs_combine_kernel, dim3((ncol + RED_BLOCK - 1) / RED_BLOCK), dim3(RED_BLOCK), 0, st, out, partial, nb, ncol, 0u);
    return hipGetLastError();
}

}  // namespace ti
