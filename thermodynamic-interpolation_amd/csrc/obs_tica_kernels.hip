// obs_tica_kernels.hip -- time-lagged independent component analysis (include/ti_hip.h ti_obs_tica_moments, ti_obs_tica_fit,
// ti_obs_tica_transform): the lagged moments of many trajectories in fp64 on the matrix cores, the whitening algebra around the
// two Jacobi solves of obs_eig_kernels.hip, and the projection.
//
// Feature pass, once per call: F [n][D] fp64, D = d rounded up to 16, pad columns 0; encode: column 2k = cos x_k, 2k + 1 = sin x_k
// (fp64 sincos of the fp32 value), else column k = x_k.  Every block also leaves the smallest row with a non-finite value it met
// (a barrier-and-LDS minimum, no atomics); tica_first_bad_kernel takes the minimum over the blocks.
// Contraction, one 256-thread group per (lag, segment of TICA_SEG pairs): pair j of lag tau is (i, i + tau) with i = traj_off[t] +
// j - cum[t], t the trajectory whose range of the lag's cumulative pair counts holds j (a bisection, done for all pairs of the
// segment by all threads before the first fill: 32 KiB of LDS, nothing of it on a fill's critical path).  With X the first and Y
// the second rows of the segment's pairs, Sxx = X^T X and Syy = Y^T Y (upper-triangle 16 x 16
// tiles), Sxy = X^T Y (all tiles) and the column sums (the product of a first operand that is 1 in its row 0 with X or Y, so row 0
// of that tile is the sum) are real contractions on v_mfma_f64_16x16x4_f64, four pairs per K step, the tiles dealt to the four waves
// round robin.  Both table rows of 16 pairs at a time are staged through LDS; the table rows of the next 16 are in flight in
// registers while the matrix cores work on the current ones: the structure of obs_gram_kernel.  A tile's sum runs over the pairs in pair order, so a
// segment's partial is a function of (the data, traj_off, tau, the segment number) only.  The partials go to the workspace with plain
// stores; tica_reduce_kernel adds them in segment order and mirrors Sxx and Syy.  No atomics.
#include <climits>

#include "ti_internal.hpp"

namespace ti {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int TICA_BLOCK = 256, TICA_CHUNK = 16;      // pairs staged per LDS fill: 4 K steps
// doubles of padding per LDS row: LD = 2 D + 16 is 16 mod 32 doubles, so the rows q and q + 1 of a K step start 32 banks apart and a
// half-wave's 8-byte reads (rows q = 0, 1 or 2, 3; 16 consecutive doubles each) cover the 64 banks once; rows q and q + 2 share
// banks, which costs nothing because such reads issue per half-wave
constexpr int TICA_LDPAD = 16;

// f [n][D]; bad [blocks]: the smallest row of the block with a non-finite value, LLONG_MAX: none.  One thread per (row, value k < K).
__global__ __launch_bounds__(TICA_BLOCK) void tica_feature_kernel(double* __restrict__ f, long long* __restrict__ bad, const float* __restrict__ x,
                                                                 long long stride, long long cstride, long long n, int K, int encode, int D)
{
    __shared__ long long red[TICA_BLOCK];
    const int KP = encode ? D / 2 : D;                 // items per row: the pad columns are written by the items k >= K
    const long long e = (long long)blockIdx.x * TICA_BLOCK + threadIdx.x;
    long long mine = LLONG_MAX;
    if (e < n * KP) {
        const long long i = e / KP;
        const int k = (int)(e - i * KP);
        double a = 0.0, b = 0.0;
        if (k < K) {
            const float v = x[i * stride + k * cstride];
            if (!isfinite(v)) mine = i;
            if (encode) sincos((double)v, &b, &a);     // a = cos, b = sin
            else a = (double)v;
        }
        if (encode) {
            f[i * D + 2 * k] = a;
            f[i * D + 2 * k + 1] = b;
        } else {
            f[i * D + k] = a;
        }
    }
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int s = TICA_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] < red[threadIdx.x + s] ? red[threadIdx.x] : red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) bad[blockIdx.x] = red[0];
}

// out[0] = the minimum of bad [m].  One group.
__global__ __launch_bounds__(TICA_BLOCK) void tica_first_bad_kernel(long long* __restrict__ out, const long long* __restrict__ bad, long long m)
{
    __shared__ long long red[TICA_BLOCK];
    long long mine = LLONG_MAX;
    for (long long i = threadIdx.x; i < m; i += TICA_BLOCK) mine = bad[i] < mine ? bad[i] : mine;
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int s = TICA_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] < red[threadIdx.x + s] ? red[threadIdx.x] : red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// T = D / 16 column tiles.  The tiles of a segment's partial, in this order (tica_tiles(T) of them):
//   Sxx (a, b), a <= b, row by row | Syy likewise | Sxy (a, b) row by row | sum X (b) | sum Y (b)
// wave v owns the tiles v, v + 4, ...: NSLOT of them at most
template <int T>
__global__ __launch_bounds__(TICA_BLOCK) void tica_moments_kernel(TicaParams g)
{
    constexpr int D = 16 * T, NU = T * (T + 1) / 2, NT = 2 * NU + T * T + 2 * T, NSLOT = (NT + 3) / 4, LD = 2 * D + TICA_LDPAD;
    constexpr int NF = TICA_CHUNK * D / TICA_BLOCK;                     // 16-byte units of a fill per thread (= T)
    __shared__ __attribute__((aligned(16))) double zs[TICA_CHUNK * LD];       // stored through f64x2
    __shared__ int ixs[TICA_SEG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, cl = lane & 15;
    // the block's lag (local number within the launch) and segment
    int ll = 0;
    while (ll + 1 < g.n_lag && (int)blockIdx.x >= g.seg_off[ll + 1]) ++ll;
    const long long seg = (long long)blockIdx.x - g.seg_off[ll], tau = g.lag[ll];
    const long long* __restrict__ cum = g.cum + (long long)ll * (g.n_traj + 1);
    const long long np = cum[g.n_traj];
    const long long j_begin = seg * TICA_SEG, j_end = j_begin + TICA_SEG < np ? j_begin + TICA_SEG : np;
    const f64x2* __restrict__ f2 = reinterpret_cast<const f64x2*>(g.f);

    // the wave's tiles: LDS offsets of the first (row tile) and second (column tile) operand of slot s; -1: the ones operand
    int offa[NSLOT], offb[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        int t = 4 * s + wave, a = 0, oa, ob;
        if (t >= NT) t = 0;                        // no such tile: the slot is skipped below
        if (t < 2 * NU) {
            const int y = t >= NU ? D : 0;
            if (t >= NU) t -= NU;
            while (t >= T - a) { t -= T - a; ++a; }
            oa = y + 16 * a;
            ob = y + 16 * (a + t);
        } else if (t < 2 * NU + T * T) {
            t -= 2 * NU;
            a = t / T;
            oa = 16 * a;
            ob = D + 16 * (t - a * T);
        } else {
            t -= 2 * NU + T * T;
            oa = -1;
            ob = t < T ? 16 * t : D + 16 * (t - T);
        }
        offa[s] = oa < 0 ? -1 : oa + cl;
        offb[s] = ob + cl;
    }
    const double one = cl == 0 ? 1.0 : 0.0;
    f64x4 acc[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) acc[s] = f64x4{0, 0, 0, 0};

    // the first frame of every pair of the segment, once, by all threads: cum[lo] <= j < cum[lo + 1] by bisection
    for (long long j = j_begin + tid; j < j_end; j += TICA_BLOCK) {
        int lo = 0, hi = g.n_traj;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] <= j) lo = mid; else hi = mid;
        }
        ixs[j - j_begin] = (int)(g.traj_off[lo] + (j - cum[lo]));
    }
    f64x2 pre[NF];
    // both table rows of the 16 pairs from j0 on into registers (zeros past the segment's end): unit u of a fill = 16 bytes, pair
    // u / D, then X units 0 .. D / 2 - 1 and Y units D / 2 .. D - 1 of that pair
    auto fetch = [&](long long j0) {
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int u = tid + TICA_BLOCK * m, r = u / D, cu = u - r * D;
            const long long j = j0 + r, i = j < j_end ? ixs[j - j_begin] : -1;
            pre[m] = i < 0 ? f64x2{0, 0} : cu < D / 2 ? f2[i * (D / 2) + cu] : f2[(i + tau) * (D / 2) + (cu - D / 2)];
        }
    };

    __syncthreads();
    fetch(j_begin);
    for (long long j0 = j_begin; j0 < j_end; j0 += TICA_CHUNK) {
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int u = tid + TICA_BLOCK * m, r = u / D, cu = u - r * D;
            *reinterpret_cast<f64x2*>(&zs[r * LD + 2 * cu]) = pre[m];
        }
        __syncthreads();
        if (j0 + TICA_CHUNK < j_end) fetch(j0 + TICA_CHUNK);
#pragma unroll
        for (int kk = 0; kk < TICA_CHUNK / 4; ++kk) {
            const double* zr = zs + (4 * kk + q) * LD;
#pragma unroll
            for (int s = 0; s < NSLOT; ++s) {
                if (4 * s + wave < NT) {
                    const double av = offa[s] < 0 ? one : zr[offa[s]];
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, zr[offb[s]], acc[s], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg, so reg * 64 + lane is the row-major offset in the tile
    double* __restrict__ out = g.part + (long long)blockIdx.x * NT * 256;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        const int t = 4 * s + wave;
        if (t < NT) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) out[t * 256 + reg * 64 + lane] = acc[s][reg];
        }
    }
}

// sum [n_lag][2][d], cov [n_lag][3][d][d] (Sxx, Syy, Sxy) of the launch's lags = their partials added in segment order; the lower
// triangles of Sxx and Syy are the stored upper ones.  One thread per (lag, entry).
__global__ __launch_bounds__(TICA_BLOCK) void tica_reduce_kernel(TicaParams g, double* __restrict__ sum, double* __restrict__ cov, int d, int T)
{
    const int ll = blockIdx.y, per = 2 * d + 3 * d * d;
    const int e = blockIdx.x * TICA_BLOCK + threadIdx.x;
    if (e >= per) return;
    const int NU = T * (T + 1) / 2, NT = 2 * NU + T * T + 2 * T;
    int tile, off;
    double* dst;
    if (e < 2 * d) {
        const int y = e / d, k = e - y * d;
        tile = 2 * NU + T * T + y * T + (k >> 4);
        off = k & 15;                                                       // row 0 of the tile
        dst = sum + (long long)ll * 2 * d + e;
    } else {
        const int c = e - 2 * d, m = c / (d * d), kl = c - m * d * d;
        int k = kl / d, l = kl - k * d;
        dst = cov + (long long)ll * 3 * d * d + c;
        if (m < 2) {
            if (k > l) { const int t = k; k = l; l = t; }
            const int tk = k >> 4, tl = l >> 4;
            tile = m * NU + tk * T - tk * (tk - 1) / 2 + (tl - tk);
        } else {
            tile = 2 * NU + (k >> 4) * T + (l >> 4);
        }
        off = (k & 15) * 16 + (l & 15);
    }
    const double* __restrict__ src = g.part + ((long long)g.seg_off[ll] * NT + tile) * 256 + off;
    const long long nseg = g.seg_off[ll + 1] - g.seg_off[ll];
    double s = 0.0;
    for (long long sg = 0; sg < nseg; ++sg) s += src[sg * NT * 256];
    *dst = s;
}

constexpr int TICA_MAX_D = EIG_MAX_N;

// ---- the model algebra, one 256-thread group per lag

// mean [d], C00 into a [d][d][2] (re, 0) and C0t [d][d] from the moments; flag [lag] = 1 where a moment is not finite
__global__ __launch_bounds__(TICA_BLOCK) void tica_fit_prep_kernel(const long long* __restrict__ count, const double* __restrict__ sum,
                                                                  const double* __restrict__ cov, int d, double* __restrict__ mean,
                                                                  double* __restrict__ a, double* __restrict__ c0t, int* __restrict__ flag)
{
    __shared__ double mu[TICA_MAX_D];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const long long l = blockIdx.x;
    const double n2 = 2.0 * (double)count[l];
    const double* __restrict__ sx = sum + l * 2 * d;
    const double *sxx = cov + l * 3 * d * d, *syy = sxx + d * d, *sxy = syy + d * d;
    if (tid == 0) bad = 0;
    __syncthreads();
    bool ok = true;
    if (tid < d) {
        ok = isfinite(sx[tid]) && isfinite(sx[d + tid]);
        mu[tid] = (sx[tid] + sx[d + tid]) / n2;
        mean[l * d + tid] = mu[tid];
    }
    for (int e = tid; e < d * d; e += TICA_BLOCK) ok = ok && isfinite(sxx[e]) && isfinite(syy[e]) && isfinite(sxy[e]);
    if (!ok) bad = 1;                                          // plain store of one value
    __syncthreads();
    for (int e = tid; e < d * d; e += TICA_BLOCK) {
        const int k = e / d, m = e - k * d;
        const double mm = mu[k] * mu[m];
        a[(l * d * d + e) * 2] = (sxx[e] + syy[e]) / n2 - mm;
        a[(l * d * d + e) * 2 + 1] = 0.0;
        c0t[l * d * d + e] = (sxy[e] + sxy[m * d + k]) / n2 - mm;
    }
    if (tid == 0) flag[l] = bad;
}

// From the eigenpairs (w1 ascending, v1 columns) of C00: s descending, r = #{s_k > epsilon}, L = V[:, :r] / sqrt(s[:r]) (also to
// lmat [d][d], columns < r), T = C0t L, Kt = L^T T of which the upper triangle goes to rmat (row stride d, (re, 0)).  rank = r; 0
// where the first solve gave no eigenpairs, and the second solve skips such a matrix.
__global__ __launch_bounds__(TICA_BLOCK) void tica_fit_reduce_kernel(const double* __restrict__ w1, const double* __restrict__ v1,
                                                                    const int* __restrict__ status1, const double* __restrict__ c0t,
                                                                    double epsilon, int d, double* __restrict__ lmat, double* __restrict__ rmat,
                                                                    int* __restrict__ rank)
{
    extern __shared__ __attribute__((aligned(16))) double tica_lds[];
    const int tid = threadIdx.x;
    const long long l = blockIdx.x;
    if (status1[l] < 1 || status1[l] > EIG_MAX_SWEEPS) {
        if (tid == 0) rank[l] = 0;
        return;
    }
    const double* __restrict__ wm = w1 + l * d;
    const double* __restrict__ vm = v1 + l * d * d * 2;
    const double* __restrict__ cm = c0t + l * d * d;
    double *L = tica_lds, *Tm = L + d * d;
    int r = 0;
    for (int k = 0; k < d; ++k) r += wm[d - 1 - k] > epsilon ? 1 : 0;       // w1 is sorted: the first r of the descending order
    if (tid == 0) rank[l] = r;
    for (int it = tid; it < d * r; it += TICA_BLOCK) {
        const int i = it / r, k = it - i * r;
        const double x = vm[2 * (i * d + (d - 1 - k))] / sqrt(wm[d - 1 - k]);
        L[i * d + k] = x;
        lmat[l * d * d + i * d + k] = x;
    }
    __syncthreads();
    for (int it = tid; it < d * r; it += TICA_BLOCK) {
        const int i = it / r, k = it - i * r;
        double acc = 0.0;
        for (int m = 0; m < d; ++m) acc += cm[i * d + m] * L[m * d + k];
        Tm[i * d + k] = acc;
    }
    __syncthreads();
    for (int it = tid; it < r * r; it += TICA_BLOCK) {
        const int j = it / r, k = it - j * r;
        if (j > k) continue;
        double acc = 0.0;
        for (int i = 0; i < d; ++i) acc += L[i * d + j] * Tm[i * d + k];
        rmat[(l * d * d + j * d + k) * 2] = acc;
        rmat[(l * d * d + j * d + k) * 2 + 1] = 0.0;
    }
}

// ev [dim] = the eigenvalues of Kt in descending order, comp [d][dim] = L U[:, :dim], each column's entry of largest magnitude (the
// lowest index among equal ones) made positive, then times its eigenvalue if scaling; NaN at index >= rank
__global__ __launch_bounds__(TICA_BLOCK) void tica_fit_back_kernel(const double* __restrict__ lmat, const double* __restrict__ w2,
                                                                  const double* __restrict__ v2, const int* __restrict__ rank, int d, int dim,
                                                                  int scaling, double* __restrict__ ev, double* __restrict__ comp)
{
    extern __shared__ __attribute__((aligned(16))) double tica_lds[];
    __shared__ double sgn[TICA_MAX_D];
    const int tid = threadIdx.x;
    const long long l = blockIdx.x;
    const int r = rank[l], nk = dim < r ? dim : r;
    const double* __restrict__ L = lmat + l * d * d;
    const double* __restrict__ vm = v2 + l * d * d * 2;
    const double nan = __builtin_nan("");
    double* R = tica_lds;                                       // [d][dim]
    for (int it = tid; it < d * dim; it += TICA_BLOCK) {
        const int f = it / dim, k = it - f * dim;
        double acc = nan;
        if (k < nk) {
            acc = 0.0;
            for (int m = 0; m < r; ++m) acc += L[f * d + m] * vm[2 * (m * d + (r - 1 - k))];
        }
        R[it] = acc;
    }
    __syncthreads();
    if (tid < dim) {
        double s = nan, lam = nan;
        if (tid < nk) {
            lam = w2[l * d + (r - 1 - tid)];
            double best = -1.0;
            s = 1.0;
            for (int f = 0; f < d; ++f) {
                const double x = R[f * dim + tid];
                if (fabs(x) > best) { best = fabs(x); s = x < 0.0 ? -1.0 : 1.0; }
            }
            if (scaling) s *= lam;
        }
        sgn[tid] = s;
        ev[l * dim + tid] = lam;
    }
    __syncthreads();
    for (int it = tid; it < d * dim; it += TICA_BLOCK) {
        const int k = it % dim;
        comp[l * d * dim + it] = k < nk ? R[it] * sgn[k] : nan;
    }
}

// out [n_lag][B][dim]: one thread per (row, component), blockIdx.y the lag
__global__ __launch_bounds__(TICA_BLOCK) void tica_transform_kernel(float* __restrict__ out, const float* __restrict__ x, long long stride,
                                                                   long long cstride, long long B, int K, int encode, int d, int dim,
                                                                   const double* __restrict__ mean, const double* __restrict__ comp)
{
    const long long e = (long long)blockIdx.x * TICA_BLOCK + threadIdx.x, l = blockIdx.y;
    if (e >= B * dim) return;
    const long long i = e / dim;
    const int k = (int)(e - i * dim);
    const double* __restrict__ mu = mean + l * d;
    const double* __restrict__ R = comp + l * d * dim + k;
    const float* __restrict__ xi = x + i * stride;
    double y = 0.0;
    bool ok = true;
    for (int a = 0; a < K; ++a) {
        const float v = xi[a * cstride];
        ok = ok && isfinite(v);
        if (encode) {
            double s, c;
            sincos((double)v, &s, &c);
            y += (c - mu[2 * a]) * R[(2 * a) * dim];
            y += (s - mu[2 * a + 1]) * R[(2 * a + 1) * dim];
        } else {
            y += ((double)v - mu[a]) * R[a * dim];
        }
    }
    out[(l * B + i) * dim + k] = ok ? (float)y : __builtin_nanf("");
}

}  // namespace

hipError_t launch_tica_features(double* f, long long* bad, long long* first_bad, const float* x, long long stride, long long cstride, long long n,
                                int K, int encode, int D, hipStream_t st)
{
    const long long blocks = tica_feature_blocks(n, encode, D);
    hipLaunchKernelGGL(tica_feature_kernel, dim3((unsigned)blocks), dim3(TICA_BLOCK), 0, st, f, bad, x, stride, cstride, n, K, encode, D);
    hipLaunchKernelGGL(tica_first_bad_kernel, dim3(1), dim3(TICA_BLOCK), 0, st, first_bad, bad, blocks);
    return hipGetLastError();
}

hipError_t launch_tica_moments(const TicaParams& g, int T, double* sum, double* cov, int d, hipStream_t st)
{
    const dim3 grid((unsigned)g.seg_off[g.n_lag]), block(TICA_BLOCK);
    switch (T) {
    case 1: hipLaunchKernelGGL(tica_moments_kernel<1>, grid, block, 0, st, g); break;
    case 2: hipLaunchKernelGGL(tica_moments_kernel<2>, grid, block, 0, st, g); break;
    case 3: hipLaunchKernelGGL(tica_moments_kernel<3>, grid, block, 0, st, g); break;
    case 4: hipLaunchKernelGGL(tica_moments_kernel<4>, grid, block, 0, st, g); break;
    default: return hipErrorInvalidValue;
    }
    const int per = 2 * d + 3 * d * d;
    hipLaunchKernelGGL(tica_reduce_kernel, dim3((unsigned)((per + TICA_BLOCK - 1) / TICA_BLOCK), (unsigned)g.n_lag), block, 0, st, g, sum, cov, d, T);
    return hipGetLastError();
}

hipError_t launch_tica_fit_prep(const long long* count, const double* sum, const double* cov, int d, double* mean, double* a, double* c0t, int* flag,
                                int n_lag, hipStream_t st)
{
    hipLaunchKernelGGL(tica_fit_prep_kernel, dim3((unsigned)n_lag), dim3(TICA_BLOCK), 0, st, count, sum, cov, d, mean, a, c0t, flag);
    return hipGetLastError();
}

hipError_t launch_tica_fit_reduce(const double* w1, const double* v1, const int* status1, const double* c0t, double epsilon, int d, double* lmat,
                                  double* rmat, int* rank, int n_lag, hipStream_t st)
{
    hipLaunchKernelGGL(tica_fit_reduce_kernel, dim3((unsigned)n_lag), dim3(TICA_BLOCK), 2 * (size_t)d * d * sizeof(double), st, w1, v1, status1, c0t,
                       epsilon, d, lmat, rmat, rank);
    return hipGetLastError();
}

hipError_t launch_tica_fit_back(const double* lmat, const double* w2, const double* v2, const int* rank, int d, int dim, int scaling, double* ev,
                                double* comp, int n_lag, hipStream_t st)
{
    hipLaunchKernelGGL(tica_fit_back_kernel, dim3((unsigned)n_lag), dim3(TICA_BLOCK), (size_t)d * dim * sizeof(double), st, lmat, w2, v2, rank, d,
                       dim, scaling, ev, comp);
    return hipGetLastError();
}

hipError_t launch_tica_transform(float* out, const float* x, long long stride, long long cstride, long long B, int K, int encode, int d, int dim,
                                 const double* mean, const double* comp, int n_lag, hipStream_t st)
{
    const long long blocks = (B * dim + TICA_BLOCK - 1) / TICA_BLOCK;
    hipLaunchKernelGGL(tica_transform_kernel, dim3((unsigned)blocks, (unsigned)n_lag), dim3(TICA_BLOCK), 0, st, out, x, stride, cstride, B, K, encode,
                       d, dim, mean, comp);
    return hipGetLastError();
}

}  // namespace ti
