// adw_train_kernels.hip -- training FCNetMultiBeta on the velocity loss (include/ti_hip.h ti_adw_train_*): the matrix products of
// the forward pass, the data gradient and the weight gradient on v_mfma_f32_16x16x4_f32, the output gradient of the loss, the fp64
// combine of the weight-gradient slices, and clip + Adam in fp64 with the refresh of the fp32 working weights.
//
// One product kernel serves all three passes: both operands are addressed by strides, so the forward pass (a W^T), the data gradient
// (g W) and the weight gradient (g^T a, contracted over the rows) read the activations and the canonical [out][in] weights as they
// lie.  Every output element is one fmaf chain over the contraction index in order -- the instruction is that chain bit for bit -- so
// a result depends on the values alone.  The weight gradient is cut into slices of TRAIN_ROW_TILE rows (blockIdx.z), each slice
// written to its own place and the slices added in fp64 in order: no atomics anywhere.  The two sums that cancel -- a bias gradient
// (the column sum of g) and the gradient handed to beta_embed (both antithetic halves of a row) -- are taken in fp64 by kernels of
// their own.  gamma'(t) of the output gradient is the velocity loss's (vloss_device.hpp).
#include "adw_train.hpp"
#include "vloss_device.hpp"

namespace ti {

namespace {

constexpr int TR_BLOCK = 256;
constexpr int TR_KU = 8;                       // chain links per round of the product kernel
typedef float tr_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ tr_f32x4 tr_mfma(float a, float b, tr_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Four waves, each a 16 x 32 tile of C on two independent accumulators that share the A operand.  Lane l holds A(i0 + l % 16, k + l / 16),
// B(k + l / 16, j + l % 16), and in register r of an accumulator C(i0 + 4 (l / 16) + r, j + l % 16).
__global__ __launch_bounds__(TR_BLOCK) void adwtr_gemm_kernel(const TrGemm p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const long long i0 = ((long long)blockIdx.x * 4 + wave) * 16;
    if (i0 >= p.M) return;                                                  // the whole wave: there is no barrier below
    const int j0 = blockIdx.y * 32, ja = j0 + c, jb = j0 + 16 + c;
    const long long k_begin = (long long)blockIdx.z * p.ktile, k_end = min(p.Kd, k_begin + p.ktile);
    const long long ia = i0 + c;
    const bool ia_ok = ia < p.M, ja_ok = ja < p.N, jb_ok = jb < p.N;
    const float* ap = p.A + (ia_ok ? ia : 0) * p.a_si;
    const float* bpa = p.B + (long long)(ja_ok ? ja : 0) * p.b_sj;
    const float* bpb = p.B + (long long)(jb_ok ? jb : 0) * p.b_sj;
    tr_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    // TR_KU steps of the chain per round: their operands are loaded first, so the loads of a round are in flight together
    for (long long k = k_begin; k < k_end; k += 4 * TR_KU) {
        float a[TR_KU], b0[TR_KU], b1[TR_KU];
#pragma unroll
        for (int u = 0; u < TR_KU; ++u) {
            const long long kk = k + 4 * u + q;
            const bool k_ok = kk < k_end;
            a[u] = ia_ok && k_ok ? ap[kk * p.a_sk] : 0.0f;
            b0[u] = ja_ok && k_ok ? bpa[kk * p.b_sk] : 0.0f;
            b1[u] = jb_ok && k_ok ? bpb[kk * p.b_sk] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < TR_KU; ++u) {
            if (k + 4 * u >= k_end) break;                                  // uniform: the chain has exactly ceil(n / 4) links
            acc0 = tr_mfma(a[u], b0[u], acc0);
            acc1 = tr_mfma(a[u], b1[u], acc1);
        }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int j = half ? jb : ja;
        if (j >= p.N) continue;
        const tr_f32x4 acc = half ? acc1 : acc0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long i = i0 + 4 * q + r;
            if (i >= p.M) continue;
            const float v = acc[r];
            if (p.mode == TRG_FWD_ACT) {
                const float z = v + p.bias[j], sg = 1.0f / (1.0f + expf(-z)), y = z * sg;
                p.out[i * p.ldo + j] = y;
                p.out2[i * p.ldo + j] = fmaf(y, 1.0f - sg, sg);
            } else if (p.mode == TRG_FWD_LIN) p.out[i * p.ldo + j] = v + p.bias[j];
            else if (p.mode == TRG_BWD_ACT) p.out[i * p.ldo + j] = v * p.dact[i * p.ldo + j];
            else if (p.mode == TRG_BWD_LIN) p.out[i * p.ldo + j] = v;
            else {
                float* dst = p.part + (size_t)blockIdx.z * p.part_stride;
                dst[p.w_off + (size_t)i * p.Kin + j] = v;
            }
        }
    }
}

__global__ __launch_bounds__(TR_BLOCK) void adwtr_gather_kernel(float* __restrict__ dst, const float* __restrict__ src, const long long* __restrict__ idx,
                                                                long long n, long long B, int m)
{
    const long long i = (long long)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= B * m) return;
    const long long b = i / m;
    long long r = idx[b];
    if (r < 0 || r >= n) r = 0;
    dst[i] = src[r * m + (i - b * m)];
}

__global__ __launch_bounds__(TR_BLOCK) void adwtr_embed_in_kernel(float* __restrict__ e0, const float* __restrict__ beta0, const float* __restrict__ beta1,
                                                                  const float* __restrict__ t, long long B)
{
    const long long b = (long long)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (b >= B) return;
    e0[3 * b] = beta0[b]; e0[3 * b + 1] = beta1[b]; e0[3 * b + 2] = t[b];
}

__global__ __launch_bounds__(TR_BLOCK) void adwtr_net_in_kernel(float* __restrict__ a0, const float* __restrict__ xt, const float* __restrict__ t,
                                                                const float* __restrict__ emb, long long B, int halves, int d)
{
    const int K = d + 2;
    const long long i = (long long)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= (long long)halves * B * K) return;
    const long long r = i / K, b = r % B;
    const int cc = (int)(i - r * K);
    a0[i] = cc < d ? xt[r * d + cc] : cc == d ? t[b] : emb[b];
}

__global__ __launch_bounds__(TR_BLOCK) void adwtr_gout_kernel(float* __restrict__ gz, const VlossParams p)
{
#pragma clang fp contract(off)
    const long long n = p.B * p.m, i = (long long)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long b = i / p.m;
    const double d = (double)p.x1[i] - (double)p.x0[i], inv = (double)p.B;
    if (p.kind == TI_VLOSS_ONE_SIDED) { gz[i] = (float)(((double)p.b[i] - d) / inv); return; }
    const double gzv = vl_gamma_dot(p.gamma, p.a, (double)p.t[b]) * (double)p.z[i];
    gz[i] = (float)(((double)p.b[i] - (d + gzv)) / inv);
    gz[n + i] = (float)(((double)p.b[p.half + i] - (d - gzv)) / inv);
}

// The gradient at beta_embed's output: the embedding column of net.0's input gradient, sum_n W0[n][K - 1] gz0[r][n], of both halves of
// row b.  It is a cancelling sum -- the halves are antithetic -- so it is taken in fp64, g+ + g- first, n in order, and rounded once.
__global__ __launch_bounds__(TR_BLOCK) void adwtr_embed_gout_kernel(float* __restrict__ ge, const float* __restrict__ gz0, const float* __restrict__ w0,
                                                                    long long B, int halves, int H, int K)
{
#pragma clang fp contract(off)
    const long long b = (long long)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int n = 0; n < H; ++n) {
        double g = (double)gz0[b * H + n];
        if (halves == 2) g = g + (double)gz0[(B + b) * H + n];
        s = s + (double)w0[(size_t)n * K + K - 1] * g;
    }
    ge[b] = (float)s;
}

// The bias gradient of a layer, db[n] = sum over the rows of gz[r][n], in fp64: accumulator p of column n adds rows p, p + 16, .. in
// order from +0.0, and the 16 accumulators are added in order.  One block per 64 columns.
constexpr int TR_BIAS_ACC = 16;
__global__ __launch_bounds__(64 * TR_BIAS_ACC) void adwtr_bias_kernel(double* __restrict__ db, const float* __restrict__ gz, long long rows, int N)
{
#pragma clang fp contract(off)
    __shared__ double sm[TR_BIAS_ACC][64];
    const int c = threadIdx.x & 63, p = threadIdx.x >> 6, n = blockIdx.x * 64 + c;
    double s = 0.0;
    if (n < N)
        for (long long r = p; r < rows; r += TR_BIAS_ACC) s = s + (double)gz[r * N + n];
    sm[p][c] = s;
    __syncthreads();
    if (p == 0 && n < N) {
        double t = 0.0;
        for (int q = 0; q < TR_BIAS_ACC; ++q) t = t + sm[q][c];
        db[n] = t;
    }
}

__global__ __launch_bounds__(TR_BLOCK) void adwtr_combine_kernel(double* __restrict__ grad, double* __restrict__ sq, const float* __restrict__ part,
                                                                 const unsigned char* __restrict__ is_bias, size_t part_stride, size_t n,
                                                                 size_t n_embed, int tiles_e, int tiles_n)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n) return;
    double g;
    if (part && !is_bias[i]) {
        const int tiles = i < n_embed ? tiles_e : tiles_n;
        g = 0.0;
        for (int z = 0; z < tiles; ++z) g += (double)part[(size_t)z * part_stride + i];
        grad[i] = g;
    } else g = grad[i];
    sq[i] = g * g;
}

// what every thread of the optimiser derives from the two batch-wide sums: skipped or not, and the clip coefficient
__device__ __forceinline__ bool tr_decide(const TrAdam& a, double& coef, double& mean)
{
#pragma clang fp contract(off)
    const double ss = a.sumsq[0];
    mean = a.loss_sum ? a.loss_sum[0] / a.B : 0.0;
    coef = 1.0;
    if (!(isfinite(ss) && isfinite(mean))) return false;
    if (a.max_norm > 0.0 && isfinite(a.max_norm)) coef = fmin(1.0, a.max_norm / (sqrt(ss) + 1e-6));
    return true;
}

__global__ __launch_bounds__(TR_BLOCK) void adwtr_adam_kernel(const TrAdam a)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    double coef, mean;
    if (!tr_decide(a, coef, mean)) return;
    const long long s = a.ctr[0] - a.base;
    const double step_size = a.bias[2 * s], bc2_sqrt = a.bias[2 * s + 1];
    const double p = a.w[i];
    double g = coef * a.grad[i];
    if (a.weight_decay != 0.0) g = g + a.weight_decay * p;
    const double m = a.beta1 * a.m[i] + (1.0 - a.beta1) * g;
    const double v = a.beta2 * a.v[i] + (1.0 - a.beta2) * (g * g);
    const double pn = p - step_size * (m / (sqrt(v) / bc2_sqrt + a.eps));
    a.m[i] = m; a.v[i] = v; a.w[i] = pn; a.w32[i] = (float)pn;
}

// after the optimiser launch: the counters it read, and the log entry of the step
__global__ void adwtr_finish_kernel(const TrAdam a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double coef, mean;
    const bool ok = tr_decide(a, coef, mean);
    const long long s = (a.ctr[0] - a.base) + (a.ctr[1] - a.base_skip);      // the step of this call
    if (ok) a.ctr[0] += 1; else a.ctr[1] += 1;
    if (a.log) a.log[s] = ok ? mean : __longlong_as_double(0x7ff8000000000000LL);
}

__global__ __launch_bounds__(TR_BLOCK) void adwtr_refresh_kernel(float* __restrict__ w32, const double* __restrict__ w, size_t n)
{
    const size_t i = (size_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i < n) w32[i] = (float)w[i];
}

unsigned tr_blocks(long long n) { return (unsigned)((n + TR_BLOCK - 1) / TR_BLOCK); }

}  // namespace

hipError_t launch_train_gemm(const TrGemm& g, int slices, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_gemm_kernel, dim3((unsigned)((g.M + 63) / 64), (unsigned)((g.N + 31) / 32), (unsigned)slices), dim3(TR_BLOCK), 0, st, g);
    return hipGetLastError();
}

hipError_t launch_train_gather(float* dst, const float* src, const long long* idx, long long n, long long B, int m, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_gather_kernel, dim3(tr_blocks(B * m)), dim3(TR_BLOCK), 0, st, dst, src, idx, n, B, m);
    return hipGetLastError();
}

hipError_t launch_train_embed_in(float* e0, const float* beta0, const float* beta1, const float* t, long long B, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_embed_in_kernel, dim3(tr_blocks(B)), dim3(TR_BLOCK), 0, st, e0, beta0, beta1, t, B);
    return hipGetLastError();
}

hipError_t launch_train_net_in(float* a0, const float* xt, const float* t, const float* emb, long long B, int halves, int d, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_net_in_kernel, dim3(tr_blocks((long long)halves * B * (d + 2))), dim3(TR_BLOCK), 0, st, a0, xt, t, emb, B, halves, d);
    return hipGetLastError();
}

hipError_t launch_train_gout(float* gz, const VlossParams& p, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_gout_kernel, dim3(tr_blocks(p.B * p.m)), dim3(TR_BLOCK), 0, st, gz, p);
    return hipGetLastError();
}

hipError_t launch_train_embed_gout(float* ge, const float* gz0, const float* w0, long long B, int halves, int H, int K, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_embed_gout_kernel, dim3(tr_blocks(B)), dim3(TR_BLOCK), 0, st, ge, gz0, w0, B, halves, H, K);
    return hipGetLastError();
}

hipError_t launch_train_bias(double* db, const float* gz, long long rows, int N, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_bias_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64 * TR_BIAS_ACC), 0, st, db, gz, rows, N);
    return hipGetLastError();
}

hipError_t launch_train_combine(double* grad, double* sq, const float* part, const unsigned char* is_bias, size_t part_stride, size_t n,
                                size_t n_embed, int tiles_e, int tiles_n, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_combine_kernel, dim3(tr_blocks((long long)n)), dim3(TR_BLOCK), 0, st, grad, sq, part, is_bias, part_stride, n, n_embed,
                       tiles_e, tiles_n);
    return hipGetLastError();
}

hipError_t launch_train_adam(const TrAdam& a, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_adam_kernel, dim3(tr_blocks((long long)a.n)), dim3(TR_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_train_finish(const TrAdam& a, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_finish_kernel, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_train_refresh(float* w32, const double* w, size_t n, hipStream_t st)
{
    hipLaunchKernelGGL(adwtr_refresh_kernel, dim3(tr_blocks((long long)n)), dim3(TR_BLOCK), 0, st, w32, w, n);
    return hipGetLastError();
}

}  // namespace ti
