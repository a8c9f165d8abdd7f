// obs_gram_kernels.hip -- random-Fourier-feature Gram matrices of bootstrap resamples (include/ti_hip.h ti_obs_rff_gram): the
// O(m p^2) part of reversible generator EDMD (the reference's gedmd/rff.py spectral_analysis_rff_generator), in fp64.
//
// Feature pass, once per call: Z [n][2P] = (cos theta | sin theta), theta_nk = sum_i x_ni Omega_ik in fp64, P = p rounded up to 16,
// pad columns 0; w_n = exp(logw_n - max logw).
// Gram pass, one 256-thread group per (resample row, segment of GRAM_SEG draws): with M = c - i s,
//   Re (M^H diag(w) M)_kl = sum_j w (c_k c_l + s_k s_l)      Im (...)_kl = sum_j w (s_k c_l - c_k s_l)
// over the segment's draws j, as real contractions on v_mfma_f64_16x16x4_f64: four draws per K step, the A operand scaled by w, the
// upper-triangle 16 x 16 tiles only, dealt to the four waves round robin.  The table rows of 16 draws at a time are gathered into
// LDS; the next 16 are in flight in registers while the matrix cores work on the current ones.  A tile's sum runs over the draws in
// draw order, so a row's partial Gram is a function of (its draws, the data, Omega, n_draw) only.  The partials go to the workspace
// with plain stores and obs_gram_reduce_kernel adds them in segment order, writes the upper triangle and mirrors it (conjugate)
// below the diagonal.  No atomics.
// More than 8 column tiles (128 < p <= 1024, ti_obs_rff_gram_wide) do not fit one group's registers: obs_gram_wide_kernel below cuts
// them into panel pairs, sums every tile by the same statement (gram_tile_step) and feeds the same reduce kernel.
#include "boot_draw.hpp"

namespace ti {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int GRAM_BLOCK = 256, GRAM_CHUNK = 16;      // draws gathered per LDS fill: 4 K steps
constexpr int GRAM_LDPAD = 16;                        // doubles of padding per LDS row: the 4 rows of a K step fall on distinct banks

// z [n][2P], w [n] (w == NULL: not written).  One thread per (sample, column < P).
__global__ __launch_bounds__(GRAM_BLOCK) void obs_gram_feature_kernel(double* __restrict__ z, double* __restrict__ w, const float* __restrict__ x,
                                                                     long long stride, long long n, int d, int p, int P,
                                                                     const double* __restrict__ omega, const float* __restrict__ logw,
                                                                     const double* __restrict__ mx)
{
    const long long e = (long long)blockIdx.x * GRAM_BLOCK + threadIdx.x;
    if (e >= n * P) return;
    const long long i = e / P;
    const int k = (int)(e - i * P);
    double c = 0.0, s = 0.0;
    if (k < p) {
        const float* __restrict__ xi = x + i * stride;
        double th = 0.0;
        for (int a = 0; a < d; ++a) th = fma((double)xi[a], omega[a * p + k], th);
        sincos(th, &s, &c);
    }
    z[i * 2 * P + k] = c;
    z[i * 2 * P + P + k] = s;
    if (w && k == 0) w[i] = exp((double)logw[i] - mx[0]);
}

// four draws of one tile: Re += (w c_k) c_l + (w s_k) s_l, Im += (w s_k) c_l - (w c_k) s_l, in this order
__device__ __forceinline__ void gram_tile_step(double w, double ac, double as, double bc, double bs, f64x4& re, f64x4& im)
{
    const double wc = w * ac, wsn = w * as;
    re = __builtin_amdgcn_mfma_f64_16x16x4f64(wc, bc, re, 0, 0, 0);
    re = __builtin_amdgcn_mfma_f64_16x16x4f64(wsn, bs, re, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f64_16x16x4f64(wsn, bc, im, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f64_16x16x4f64(-wc, bs, im, 0, 0, 0);
}

// T = P / 16 column tiles, NT = T (T + 1) / 2 upper-triangle tiles; wave v owns the tiles v, v + 4, ...: NSLOT of them at most
template <int T>
__global__ __launch_bounds__(GRAM_BLOCK) void obs_gram_kernel(GramParams g)
{
    constexpr int P = 16 * T, NT = T * (T + 1) / 2, NSLOT = (NT + 3) / 4, LD = 2 * P + GRAM_LDPAD;
    constexpr int NU = GRAM_CHUNK * P / GRAM_BLOCK;                     // 16-byte units of a fill per thread (= T)
    __shared__ double zs[GRAM_CHUNK * LD];
    __shared__ double ws[GRAM_CHUNK];
    __shared__ int ixs[2][GRAM_CHUNK];
    const BootParams& p = g.draw;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, cl = lane & 15;
    const long long row = blockIdx.x / g.nseg, seg = blockIdx.x - row * g.nseg, nd = p.n_draw;
    const long long j_begin = seg * GRAM_SEG, j_end = j_begin + GRAM_SEG < nd ? j_begin + GRAM_SEG : nd;
    const uint64_t R = (uint64_t)p.first + (uint64_t)row;
    const f64x2* __restrict__ z2 = reinterpret_cast<const f64x2*>(g.z);
    bool ok = true;

    // the wave's tiles: LDS offsets of the A (row tile) and B (column tile) operands of slot s
    int offa[NSLOT], offb[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        int t = 4 * s + wave, ti = 0;
        if (t >= NT) t = 0;                        // no such tile: the slot is skipped below
        while (t >= T - ti) { t -= T - ti; ++ti; }
        offa[s] = 16 * ti + cl;
        offb[s] = 16 * (ti + t) + cl;
    }
    f64x4 re[NSLOT], im[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) { re[s] = f64x4{0, 0, 0, 0}; im[s] = f64x4{0, 0, 0, 0}; }

    // population indices of the 16 draws from j0 on into ixs[b] (-1: past the segment's end), by the first 8 threads
    auto draw = [&](long long j0, int b) {
        if (tid < GRAM_CHUNK / 2) {
            const long long j = j0 + 2 * tid;
            long long i0 = -1, i1 = -1;
            if (j < j_end) {
                boot_draw_pair(p, row, R, j >> 1, i0, i1, ok);
                if (j + 1 >= j_end) i1 = -1;
            }
            ixs[b][2 * tid] = (int)i0;
            ixs[b][2 * tid + 1] = (int)i1;
        }
    };
    f64x2 pre[NU];
    double prew = 0.0;
    // the table rows (and weights) of the draws in ixs[b] into registers: unit u of a fill = 16 bytes, row u / P, columns 2 (u % P)
    auto fetch = [&](int b) {
#pragma unroll
        for (int m = 0; m < NU; ++m) {
            const int u = tid + GRAM_BLOCK * m, r = u / P, cu = u - r * P;
            const int i = ixs[b][r];
            pre[m] = i >= 0 ? z2[(long long)i * P + cu] : f64x2{0, 0};
        }
        if (tid < GRAM_CHUNK) {
            const int i = ixs[b][tid];
            prew = i < 0 ? 0.0 : g.w ? g.w[i] : 1.0;
        }
    };

    draw(j_begin, 0);
    __syncthreads();
    fetch(0);
    int b = 0;
    for (long long j0 = j_begin; j0 < j_end; j0 += GRAM_CHUNK, b ^= 1) {
#pragma unroll
        for (int m = 0; m < NU; ++m) {
            const int u = tid + GRAM_BLOCK * m, r = u / P, cu = u - r * P;
            *reinterpret_cast<f64x2*>(&zs[r * LD + 2 * cu]) = pre[m];
        }
        if (tid < GRAM_CHUNK) ws[tid] = prew;
        const bool more = j0 + GRAM_CHUNK < j_end;
        if (more) draw(j0 + GRAM_CHUNK, b ^ 1);
        __syncthreads();
        if (more) fetch(b ^ 1);
#pragma unroll
        for (int kk = 0; kk < GRAM_CHUNK / 4; ++kk) {
            const int r = 4 * kk + q;
            const double w = ws[r];
            const double* zr = zs + r * LD;
#pragma unroll
            for (int s = 0; s < NSLOT; ++s) {
                if (4 * s + wave < NT) {
                    gram_tile_step(w, zr[offa[s]], zr[P + offa[s]], zr[offb[s]], zr[P + offb[s]], re[s], im[s]);
                }
            }
        }
        __syncthreads();
    }
    if (!ok) *p.flag = 1;                       // plain store of one value: whoever writes, the flag reads 1

    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg, so reg * 64 + lane is the row-major offset in the tile
    double* __restrict__ out = g.part + (long long)blockIdx.x * NT * 512;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        const int t = 4 * s + wave;
        if (t < NT) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                out[t * 512 + reg * 64 + lane] = re[s][reg];
                out[t * 512 + 256 + reg * 64 + lane] = im[s][reg];
            }
        }
    }
}

// ---- the blocked pass, 128 < p <= 1024 (ti_obs_rff_gram_wide)
// The T column tiles are cut into panels of GRAM_PANEL = 8 (the last may be narrower); one group per (resample row, segment, panel
// pair I <= J).  A diagonal pair accumulates the upper-triangle tiles of its panel, an off-diagonal pair all T_I T_J tiles: at most 64,
// 16 per wave, dealt round robin as above.  Both panels of the 16 gathered draws sit in LDS, a row laid out (cos I | sin I | cos J |
// sin J).  A tile's sum is gram_tile_step over the segment's draws in draw order, chunk boundaries included: the statement
// obs_gram_kernel<T> makes, so a tile holds the bits that kernel gives for its pair of column tiles.  The partial of tile (k, l)
// goes to the slot obs_gram_reduce_kernel reads it from, the upper-triangle number of the whole matrix.
// Only the last panel can be narrow, so the widths are template arguments -- DIAG: panel I = J of TJ tiles; else panel I of 8 tiles
// and panel J of TJ -- and a launch covers the pairs of one shape (launch_obs_gram_wide).
constexpr int GRAM_PANEL = 8;

// grid = rows * nseg * cnt; pair c < cnt of a (row, segment) is, DIAG: (pi0 + c, pi0 + c); else with jfix >= 0: (c, jfix); else pair c
// of the I < J among the first pi0 panels, row by row
template <int TJ, bool DIAG>
__global__ __launch_bounds__(GRAM_BLOCK) void obs_gram_wide_kernel(GramParams g, int pi0, int jfix, int cnt)
{
    constexpr int TI = DIAG ? TJ : GRAM_PANEL, WI = 16 * TI, WJ = 16 * TJ, OJ = DIAG ? 0 : 2 * WI;   // OJ: where panel J starts in an LDS row
    constexpr int NT = DIAG ? TJ * (TJ + 1) / 2 : TI * TJ, NSLOT = (NT + 3) / 4, LD = OJ + 2 * WJ + GRAM_LDPAD;
    __shared__ double zs[GRAM_CHUNK * LD];
    __shared__ double ws[GRAM_CHUNK];
    __shared__ int ixs[2][GRAM_CHUNK];
    const BootParams& p = g.draw;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, cl = lane & 15;
    const int T = g.T, P = 16 * T;
    const long long rs = blockIdx.x / cnt, row = rs / g.nseg, seg = rs - row * g.nseg, nd = p.n_draw;
    int pi = (int)(blockIdx.x - rs * cnt), pj;
    if (DIAG) { pi += pi0; pj = pi; }
    else if (jfix >= 0) pj = jfix;
    else {
        int c = pi;
        pi = 0;
        while (c >= pi0 - 1 - pi) { c -= pi0 - 1 - pi; ++pi; }
        pj = pi + 1 + c;
    }
    const long long j_begin = seg * GRAM_SEG, j_end = j_begin + GRAM_SEG < nd ? j_begin + GRAM_SEG : nd;
    const uint64_t R = (uint64_t)p.first + (uint64_t)row;
    const f64x2* __restrict__ z2 = reinterpret_cast<const f64x2*>(g.z);
    bool ok = true;

    // the wave's tiles: slot s is tile t = 4 s + wave of the pair, (a, b) = row tile of panel I, column tile of panel J -- the upper
    // triangle row by row on the diagonal, the TI x TJ rectangle row by row off it; LDS offsets of its A and B operands
    int ta[NSLOT], tb[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        int t = 4 * s + wave, a = 0;
        if (t >= NT) t = 0;                        // no such tile: the slot is skipped below
        if (DIAG) {
            while (t >= TJ - a) { t -= TJ - a; ++a; }
            t += a;
        } else {
            a = t / TJ;
            t -= a * TJ;
        }
        ta[s] = a;
        tb[s] = t;
    }
    f64x4 re[NSLOT], im[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) { re[s] = f64x4{0, 0, 0, 0}; im[s] = f64x4{0, 0, 0, 0}; }

    // population indices of the 16 draws from j0 on into ixs[b] (-1: past the segment's end), by the first 8 threads
    auto draw = [&](long long j0, int b) {
        if (tid < GRAM_CHUNK / 2) {
            const long long j = j0 + 2 * tid;
            long long i0 = -1, i1 = -1;
            if (j < j_end) {
                boot_draw_pair(p, row, R, j >> 1, i0, i1, ok);
                if (j + 1 >= j_end) i1 = -1;
            }
            ixs[b][2 * tid] = (int)i0;
            ixs[b][2 * tid + 1] = (int)i1;
        }
    };
    // a fill: 16 threads per draw; unit v = fc + 16 m of a panel of t tiles is 16 bytes, the cos columns 2 v for v < 8 t, else the
    // sin columns 2 (v - 8 t); a thread takes the units m < t of each panel
    const int fr = tid >> 4, fc = tid & 15;
    f64x2 prei[TI], prej[DIAG ? 1 : TJ];
    double prew = 0.0;
    auto fetch = [&](int b) {
        const int i = ixs[b][fr];
        const f64x2* __restrict__ zi = z2 + (long long)(i < 0 ? 0 : i) * P + (GRAM_PANEL * 8) * pi;
        const f64x2* __restrict__ zj = z2 + (long long)(i < 0 ? 0 : i) * P + (GRAM_PANEL * 8) * pj;
#pragma unroll
        for (int m = 0; m < TI; ++m) {
            const int v = fc + 16 * m;
            prei[m] = i >= 0 ? zi[v < 8 * TI ? v : P / 2 + v - 8 * TI] : f64x2{0, 0};
        }
        if (!DIAG) {
#pragma unroll
            for (int m = 0; m < TJ; ++m) {
                const int v = fc + 16 * m;
                prej[m] = i >= 0 ? zj[v < 8 * TJ ? v : P / 2 + v - 8 * TJ] : f64x2{0, 0};
            }
        }
        if (tid < GRAM_CHUNK) {
            const int iw = ixs[b][tid];
            prew = iw < 0 ? 0.0 : g.w ? g.w[iw] : 1.0;
        }
    };

    draw(j_begin, 0);
    __syncthreads();
    fetch(0);
    int b = 0;
    for (long long j0 = j_begin; j0 < j_end; j0 += GRAM_CHUNK, b ^= 1) {
#pragma unroll
        for (int m = 0; m < TI; ++m) {
            const int v = fc + 16 * m;
            *reinterpret_cast<f64x2*>(&zs[fr * LD + (v < 8 * TI ? 2 * v : WI + 2 * (v - 8 * TI))]) = prei[m];
        }
        if (!DIAG) {
#pragma unroll
            for (int m = 0; m < TJ; ++m) {
                const int v = fc + 16 * m;
                *reinterpret_cast<f64x2*>(&zs[fr * LD + OJ + (v < 8 * TJ ? 2 * v : WJ + 2 * (v - 8 * TJ))]) = prej[m];
            }
        }
        if (tid < GRAM_CHUNK) ws[tid] = prew;
        const bool more = j0 + GRAM_CHUNK < j_end;
        if (more) draw(j0 + GRAM_CHUNK, b ^ 1);
        __syncthreads();
        if (more) fetch(b ^ 1);
#pragma unroll
        for (int kk = 0; kk < GRAM_CHUNK / 4; ++kk) {
            const int r = 4 * kk + q;
            const double w = ws[r];
            const double* zr = zs + r * LD + cl;
#pragma unroll
            for (int s = 0; s < NSLOT; ++s)
                if (4 * s + wave < NT)
                    gram_tile_step(w, zr[16 * ta[s]], zr[WI + 16 * ta[s]], zr[OJ + 16 * tb[s]], zr[OJ + WJ + 16 * tb[s]], re[s], im[s]);
        }
        __syncthreads();
    }
    if (!ok) *p.flag = 1;                       // plain store of one value: whoever writes, the flag reads 1

    // tile (k, l) of the whole matrix, k <= l, is partial tile k T - k (k - 1) / 2 + (l - k) of this (row, segment)
    double* __restrict__ out = g.part + rs * ((long long)T * (T + 1) / 2) * 512;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        if (4 * s + wave < NT) {
            const int k = GRAM_PANEL * pi + ta[s], l = GRAM_PANEL * pj + tb[s];
            double* __restrict__ o = out + (long long)(k * T - k * (k - 1) / 2 + (l - k)) * 512;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                o[reg * 64 + lane] = re[s][reg];
                o[256 + reg * 64 + lane] = im[s][reg];
            }
        }
    }
}

// out [rows][p][p][2]: entry (k, l), k <= l, = the sum over the nseg partials of its row in segment order; (l, k) its conjugate;
// the imaginary part of the diagonal is 0.  One thread per (row, k, l).
__global__ __launch_bounds__(GRAM_BLOCK) void obs_gram_reduce_kernel(double* __restrict__ out, const double* __restrict__ part, long long rows,
                                                                    long long nseg, int p, int T)
{
    const long long e = (long long)blockIdx.x * GRAM_BLOCK + threadIdx.x;
    if (e >= rows * p * p) return;
    const long long row = e / (p * p);
    const int kl = (int)(e - row * p * p), k = kl / p, l = kl - k * p;
    if (k > l) return;
    const int tk = k >> 4, tl = l >> 4, NT = T * (T + 1) / 2;
    const int t = tk * T - tk * (tk - 1) / 2 + (tl - tk);
    const double* __restrict__ src = part + (row * nseg * NT + t) * 512 + (k & 15) * 16 + (l & 15);
    double sr = 0.0, si = 0.0;
    for (long long s = 0; s < nseg; ++s) {
        sr += src[s * NT * 512];
        si += src[s * NT * 512 + 256];
    }
    if (k == l) si = 0.0;
    double* __restrict__ o = out + row * p * p * 2;
    o[(k * p + l) * 2] = sr;
    o[(k * p + l) * 2 + 1] = si;
    if (k != l) {
        o[(l * p + k) * 2] = sr;
        o[(l * p + k) * 2 + 1] = -si;
    }
}

}  // namespace

hipError_t launch_obs_gram_features(double* z, double* w, const float* x, long long stride, long long n, int d, int p, const double* omega,
                                    const float* logw, const double* mx, hipStream_t st)
{
    const int P = gram_pad(p);
    const long long blocks = (n * P + GRAM_BLOCK - 1) / GRAM_BLOCK;
    hipLaunchKernelGGL(obs_gram_feature_kernel, dim3((unsigned)blocks), dim3(GRAM_BLOCK), 0, st, z, logw ? w : nullptr, x, stride, n, d, p, P, omega,
                       logw, mx);
    return hipGetLastError();
}

hipError_t launch_obs_gram(const GramParams& g, long long n_rows, hipStream_t st)
{
    const dim3 grid((unsigned)(n_rows * g.nseg)), block(GRAM_BLOCK);
    switch (g.T) {
    case 1: hipLaunchKernelGGL(obs_gram_kernel<1>, grid, block, 0, st, g); break;
    case 2: hipLaunchKernelGGL(obs_gram_kernel<2>, grid, block, 0, st, g); break;
    case 3: hipLaunchKernelGGL(obs_gram_kernel<3>, grid, block, 0, st, g); break;
    case 4: hipLaunchKernelGGL(obs_gram_kernel<4>, grid, block, 0, st, g); break;
    case 5: hipLaunchKernelGGL(obs_gram_kernel<5>, grid, block, 0, st, g); break;
    case 6: hipLaunchKernelGGL(obs_gram_kernel<6>, grid, block, 0, st, g); break;
    case 7: hipLaunchKernelGGL(obs_gram_kernel<7>, grid, block, 0, st, g); break;
    case 8: hipLaunchKernelGGL(obs_gram_kernel<8>, grid, block, 0, st, g); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

namespace {

template <bool DIAG>
hipError_t launch_gram_wide_shape(int tj, const GramParams& g, long long rs, int pi0, int jfix, int cnt, hipStream_t st)
{
    const long long blocks = rs * cnt;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(GRAM_BLOCK);
    switch (tj) {
    case 1: hipLaunchKernelGGL((obs_gram_wide_kernel<1, DIAG>), grid, block, 0, st, g, pi0, jfix, cnt); break;
    case 2: hipLaunchKernelGGL((obs_gram_wide_kernel<2, DIAG>), grid, block, 0, st, g, pi0, jfix, cnt); break;
    case 3: hipLaunchKernelGGL((obs_gram_wide_kernel<3, DIAG>), grid, block, 0, st, g, pi0, jfix, cnt); break;
    case 4: hipLaunchKernelGGL((obs_gram_wide_kernel<4, DIAG>), grid, block, 0, st, g, pi0, jfix, cnt); break;
    case 5: hipLaunchKernelGGL((obs_gram_wide_kernel<5, DIAG>), grid, block, 0, st, g, pi0, jfix, cnt); break;
    case 6: hipLaunchKernelGGL((obs_gram_wide_kernel<6, DIAG>), grid, block, 0, st, g, pi0, jfix, cnt); break;
    case 7: hipLaunchKernelGGL((obs_gram_wide_kernel<7, DIAG>), grid, block, 0, st, g, pi0, jfix, cnt); break;
    case 8: hipLaunchKernelGGL((obs_gram_wide_kernel<8, DIAG>), grid, block, 0, st, g, pi0, jfix, cnt); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

// nf full panels and, if T is no multiple of 8, a last one of tl tiles: the full diagonal pairs, the last diagonal pair, the pairs of
// two full panels, the pairs of a full panel and the last -- every upper-triangle tile of the matrix in exactly one launch
hipError_t launch_obs_gram_wide(const GramParams& g, long long n_rows, hipStream_t st)
{
    if (g.T <= GRAM_PANEL || g.T > GRAM_WIDE_MAX_P / 16) return hipErrorInvalidValue;
    const int nf = g.T / GRAM_PANEL, tl = g.T % GRAM_PANEL;
    const long long rs = n_rows * g.nseg;
    hipError_t e = launch_gram_wide_shape<true>(GRAM_PANEL, g, rs, 0, -1, nf, st);
    if (e == hipSuccess && tl) e = launch_gram_wide_shape<true>(tl, g, rs, nf, -1, 1, st);
    if (e == hipSuccess && nf > 1) e = launch_gram_wide_shape<false>(GRAM_PANEL, g, rs, nf, -1, nf * (nf - 1) / 2, st);
    if (e == hipSuccess && tl) e = launch_gram_wide_shape<false>(tl, g, rs, nf, nf, nf, st);
    return e;
}

hipError_t launch_obs_gram_reduce(double* out, const double* part, long long n_rows, long long nseg, int p, hipStream_t st)
{
    const long long blocks = (n_rows * p * p + GRAM_BLOCK - 1) / GRAM_BLOCK;
    hipLaunchKernelGGL(obs_gram_reduce_kernel, dim3((unsigned)blocks), dim3(GRAM_BLOCK), 0, st, out, part, n_rows, nseg, p, gram_pad(p) / 16);
    return hipGetLastError();
}

}  // namespace ti
