// obs_zmat_kernels.hip -- Z-matrix coordinates (include/ti_hip.h ti_obs_zmat, ti_obs_zmat_xyz) and the histograms of all columns of
// a value array in one launch (ti_obs_hist_cols).  Arithmetic is fp64 on the fp32 inputs, no atomics.  A molecule's outputs are
// computed by one thread from its own inputs and the topology, so they do not depend on its place in the batch; the batch-wide sums
// of the histograms are per-block partials in the fixed tree and trip order of obs_kernels.hip, combined block by block.
// The geometry helpers and the DIST / ANGLE / TORSION expressions restate those of obs_kernels.hip (obs_cv_kernel) term by term:
// ti_obs_zmat returns the bits ti_obs_cv returns for the equivalent descriptors.  bin_of and the trip structure of the histogram
// kernel restate obs_whist_kernel in the same way: a column's sums are taken in the order ti_obs_hist takes them.
#include "ode_device.hpp"

namespace ti {

namespace {

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 atom(const float* __restrict__ xb, int a) { return V3{(double)xb[3 * a], (double)xb[3 * a + 1], (double)xb[3 * a + 2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// ---- x -> z --------------------------------------------------------------------------------------------------------------------
// One thread per (molecule, sorted atom s >= 1).  topo: order [A] then ref [A][3] (sorted numbering), validated on the host.
__global__ __launch_bounds__(256) void obs_zmat_kernel(ZmatParams p)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int rows = p.A - 1;
    if (idx >= p.B * rows) return;
    const long long b = idx / rows;
    const int s = (int)(idx - b * rows) + 1;
    const int32_t* __restrict__ order = p.topo;
    const int32_t* __restrict__ r = p.topo + p.A + 3 * s;
    const float* __restrict__ xb = p.x + b * (3 * p.A);
    const int i4 = order[s], i3 = order[r[0]];
    double d, a = 0.0, t = 0.0;
    {                                                        // DIST(s, r1): |x_j - x_i|
        const V3 v = sub(atom(xb, i3), atom(xb, i4));
        d = sqrt(dot(v, v));
    }
    if (s >= 2) {                                            // ANGLE(s, r1, r2): the angle at r1
        const int i2 = order[r[1]];
        const V3 c = atom(xb, i3), u = sub(atom(xb, i4), c), v = sub(atom(xb, i2), c), w = cross(u, v);
        a = atan2(sqrt(dot(w, w)), dot(u, v));
        if (s >= 3) {                                        // TORSION(r3, r2, r1, s)
            const int i1 = order[r[2]];
            const V3 x1 = atom(xb, i1), x2 = atom(xb, i2), x3 = atom(xb, i3), x4 = atom(xb, i4);
            const V3 b1 = sub(x2, x1), b2 = sub(x3, x2), b3 = sub(x4, x3), c23 = cross(b2, b3);
            t = atan2(sqrt(dot(b2, b2)) * dot(b1, c23), dot(cross(b1, b2), c23));
        }
    }
    float* __restrict__ o = p.z + idx * 3;
    o[0] = (float)d; o[1] = (float)a; o[2] = (float)t;
}

// ---- z -> x (NeRF), log|det J|, validity ------------------------------------------------------------------------------------------
constexpr int ZX_BLOCK = 64;               // one wave; the placed positions of its 64 molecules take 1536 A bytes of LDS

// One thread per molecule: the chain is sequential.  The placed positions are fp64 and are indexed by ref at run time, so they live
// in LDS as pos[(3 s + c) * 64 + lane] -- a lane reads and writes its own column only, no barrier is needed.
__global__ __launch_bounds__(ZX_BLOCK) void obs_zmat_xyz_kernel(ZmatXyzParams p)
{
    extern __shared__ double pos[];
    const int lane = threadIdx.x, A = p.A;
    const long long b = (long long)blockIdx.x * ZX_BLOCK + lane;
    if (b >= p.B) return;
    const int32_t* __restrict__ order = p.topo;
    const int32_t* __restrict__ ref = p.topo + A;
    const float* __restrict__ zb = p.z + b * (3 * (A - 1));
    float* __restrict__ xb = p.x + b * (3 * A);
    auto put = [&](int s, V3 v) {
        pos[(3 * s) * ZX_BLOCK + lane] = v.x; pos[(3 * s + 1) * ZX_BLOCK + lane] = v.y; pos[(3 * s + 2) * ZX_BLOCK + lane] = v.z;
        float* __restrict__ o = xb + 3 * order[s];
        o[0] = (float)v.x; o[1] = (float)v.y; o[2] = (float)v.z;
    };
    auto get = [&](int s) { return V3{pos[(3 * s) * ZX_BLOCK + lane], pos[(3 * s + 1) * ZX_BLOCK + lane], pos[(3 * s + 2) * ZX_BLOCK + lane]}; };
    const float pi32 = 3.14159274101257324f;                 // (float)pi
    bool ok = true;
    double logdet = 0.0;
    put(0, V3{0.0, 0.0, 0.0});
    for (int s = 1; s < A; ++s) {
        const float df = zb[3 * (s - 1)], af = zb[3 * (s - 1) + 1], tf = zb[3 * (s - 1) + 2];
        ok = ok && df > 0.f && af >= 0.f && af <= pi32 && tf > -pi32 && tf <= pi32;      // a NaN fails its comparison
        const double d = (double)df, a = (double)af, t = (double)tf;
        if (s == 1) {
            put(1, V3{d, 0.0, 0.0});
        } else if (s == 2) {
            const int r1 = ref[6];
            const double x0 = r1 != 0 ? get(r1).x - d * cos(a) : d * cos(a);
            put(2, V3{x0, d * sin(a), 0.0});
            logdet += log(fabs(d));
        } else {
            const V3 p3 = get(ref[3 * s]), p2 = get(ref[3 * s + 1]), p1 = get(ref[3 * s + 2]);
            V3 e1 = sub(p3, p2);
            const double l1 = sqrt(dot(e1, e1));
            e1 = V3{e1.x / l1, e1.y / l1, e1.z / l1};
            V3 n = cross(sub(p2, p1), e1);
            const double ln = sqrt(dot(n, n));
            n = V3{n.x / ln, n.y / ln, n.z / ln};
            const V3 e2 = cross(n, e1);
            const double sa = sin(a), c1 = d * cos(a), c2 = d * sa * cos(t), c3 = d * sa * sin(t);
            put(s, V3{p3.x - c1 * e1.x + c2 * e2.x + c3 * n.x, p3.y - c1 * e1.y + c2 * e2.y + c3 * n.y, p3.z - c1 * e1.z + c2 * e2.z + c3 * n.z});
            logdet += 2.0 * log(fabs(d)) + log(fabs(sa));
        }
    }
    if (p.logdet) p.logdet[b] = logdet;
    if (p.valid) p.valid[b] = ok ? 1 : 0;
}

// ---- histograms of all columns, masked weights ------------------------------------------------------------------------------------
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

// partial [blocks][3] over the kept entries: the largest finite logw (-inf: none; logw == NULL: 0 for a kept entry), the smallest index
// of a non-finite kept logw as a double (+inf: none), the number of kept entries
__global__ __launch_bounds__(RED_BLOCK) void obs_keep_max_kernel(double* __restrict__ partial, const float* __restrict__ logw,
                                                                const uint8_t* __restrict__ keep, long long B)
{
    double mx = -HUGE_VAL, bad = HUGE_VAL, cnt = 0.0;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < B; i += (long long)gridDim.x * RED_BLOCK) {
        if (!keep[i]) continue;
        cnt += 1.0;
        const float v = logw ? logw[i] : 0.f;
        if (isfinite(v)) mx = fmax(mx, (double)v);
        else bad = fmin(bad, (double)i);
    }
    mx = block_reduce(mx, 1);
    bad = block_reduce(bad, 2);
    cnt = block_reduce(cnt, 0);
    if (threadIdx.x == 0) { partial[3 * blockIdx.x] = mx; partial[3 * blockIdx.x + 1] = bad; partial[3 * blockIdx.x + 2] = cnt; }
}

// partial [blocks]: sum w over the kept entries, w = exp(logw - m), each thread's entries in index order, then the block tree
__global__ __launch_bounds__(RED_BLOCK) void obs_keep_sum_kernel(double* __restrict__ partial, const float* __restrict__ logw,
                                                                const uint8_t* __restrict__ keep, double m, long long B)
{
    double s1 = 0.0;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < B; i += (long long)gridDim.x * RED_BLOCK)
        if (keep[i]) s1 += exp((double)logw[i] - m);
    s1 = block_reduce(s1, 0);
    if (threadIdx.x == 0) partial[blockIdx.x] = s1;
}

// out[g][c] = partial[g][0][c] op partial[g][1][c] op ... in block order, g < groups (grid y), c < ncol; op of column c: bits 2c, 2c+1
// of `ops` for c < 16 (0 sum, 1 max, 2 min), sum beyond
__global__ __launch_bounds__(RED_BLOCK) void obs_cols_combine_kernel(double* __restrict__ out, const double* __restrict__ partial, int nb, int ncol, unsigned ops)
{
    const int c = blockIdx.x * RED_BLOCK + threadIdx.x;
    if (c >= ncol) return;
    const int op = c < 16 ? (ops >> (2 * c)) & 3 : 0;
    const double* __restrict__ pg = partial + (size_t)blockIdx.y * nb * ncol;
    double acc = pg[c];
    for (int k = 1; k < nb; ++k) {
        const double v = pg[(size_t)k * ncol + c];
        acc = op == 0 ? acc + v : op == 1 ? fmax(acc, v) : fmin(acc, v);
    }
    out[(size_t)blockIdx.y * ncol + c] = acc;
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

// Grid (blocks, K): block (x, y) is block x of obs_whist_kernel on column y of values [B][K] with that column's range (lo[y], hi[y]);
// partial [K][blocks][n_bins + 3].  The weight of entry i is exp(logw[i] - m) / tot (logw == NULL: 1 / tot), 0 where keep[i] == 0.
__global__ __launch_bounds__(RED_BLOCK) void obs_whist_cols_kernel(double* __restrict__ partial, const float* __restrict__ values, int K,
                                                                  const float* __restrict__ logw, const uint8_t* __restrict__ keep, double m, double tot,
                                                                  long long B, int n_bins, const double* __restrict__ lo_c, const double* __restrict__ hi_c)
{
    __shared__ double sm[OBS_WAVES][OBS_BIN_CHUNKS * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nb = n_bins + 3, col = blockIdx.y;
    const double lo = lo_c[col], hi = hi_c[col];
    double acc[OBS_BIN_CHUNKS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long base = ((long long)blockIdx.x * OBS_WAVES + wave) * 64; base < B; base += (long long)gridDim.x * RED_BLOCK) {
        const long long i = base + lane;
        int bin = -1;
        double w = 0.0;
        if (i < B) {
            bin = bin_of(values[i * K + col], n_bins, lo, hi);
            w = (logw ? exp((double)logw[i] - m) : 1.0) / tot;
            if (keep && !keep[i]) w = 0.0;
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
    double* __restrict__ pg = partial + ((size_t)col * gridDim.x + blockIdx.x) * nb;
    for (int c = threadIdx.x; c < nb; c += RED_BLOCK) {
        double t = sm[0][c];
#pragma unroll
        for (int w2 = 1; w2 < OBS_WAVES; ++w2) t += sm[w2][c];
        pg[c] = t;
    }
}

}  // namespace

hipError_t launch_obs_zmat(const ZmatParams& p, hipStream_t st)
{
    const long long n = p.B * (p.A - 1);
    if (n > 0) hipLaunchKernelGGL(obs_zmat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_obs_zmat_xyz(const ZmatXyzParams& p, hipStream_t st)
{
    if (p.B > 0)
        hipLaunchKernelGGL(obs_zmat_xyz_kernel, dim3((unsigned)((p.B + ZX_BLOCK - 1) / ZX_BLOCK)), dim3(ZX_BLOCK),
                           (size_t)3 * p.A * ZX_BLOCK * sizeof(double), st, p);
    return hipGetLastError();
}

hipError_t launch_obs_keep_max(double* out, double* partial, const float* logw, const uint8_t* keep, long long B, hipStream_t st)
{
    const int nb = obs_blocks(B);
    hipLaunchKernelGGL(obs_keep_max_kernel, dim3(nb), dim3(RED_BLOCK), 0, st, partial, logw, keep, B);
    hipLaunchKernelGGL(obs_cols_combine_kernel, dim3(1, 1), dim3(RED_BLOCK), 0, st, out, partial, nb, 3, 1u | (2u << 2));
    return hipGetLastError();
}

hipError_t launch_obs_keep_sum(double* out, double* partial, const float* logw, const uint8_t* keep, double m, long long B, hipStream_t st)
{
    const int nb = obs_blocks(B);
    hipLaunchKernelGGL(obs_keep_sum_kernel, dim3(nb), dim3(RED_BLOCK), 0, st, partial, logw, keep, m, B);
    hipLaunchKernelGGL(obs_cols_combine_kernel, dim3(1, 1), dim3(RED_BLOCK), 0, st, out, partial, nb, 1, 0u);
    return hipGetLastError();
}

hipError_t launch_obs_whist_cols(double* out, double* partial, const float* values, int K, const float* logw, const uint8_t* keep, double m,
                                 double tot, long long B, int n_bins, const double* lo, const double* hi, hipStream_t st)
{
    const int nb = obs_blocks(B), ncol = n_bins + 3;
    hipLaunchKernelGGL(obs_whist_cols_kernel, dim3(nb, K), dim3(RED_BLOCK), 0, st, partial, values, K, logw, keep, m, tot, B, n_bins, lo, hi);
    hipLaunchKernelGGL(obs_cols_combine_kernel, dim3((ncol + RED_BLOCK - 1) / RED_BLOCK, K), dim3(RED_BLOCK), 0, st, out, partial, nb, ncol, 0u);
    return hipGetLastError();
}

}  // namespace ti
