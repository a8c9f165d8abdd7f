// adw_train.hpp -- private header of the adw trainer (include/ti_hip.h ti_adw_trainer_create .. ti_adw_train_set_lr): the state a
// trainer handle owns, and the launchers of adw_train_kernels.hip.  Shared by adw_train_kernels.hip and api_adw_train.hip only.
#pragma once
#include "ti_internal.hpp"

namespace ti {

constexpr int TRAIN_ROW_TILE = 512;         // rows per tile of the weight-gradient contraction: fixed, so a gradient does not depend on the launch
inline long long train_row_tiles(long long rows) { return (rows + TRAIN_ROW_TILE - 1) / TRAIN_ROW_TILE; }

// One matrix product C(i, j) = sum_k A(i, k) B(k, j) on v_mfma_f32_16x16x4_f32, i < M, j < N, k < Kd, both operands addressed by
// strides (element (i, k) of A at A[i a_si + k a_sk], element (k, j) of B at B[k b_sk + j b_sj]); entries outside the ranges are
// zero operands and are never read.  Every C(i, j) is one fmaf chain over k in order, from +0.0.  blockIdx.z cuts the contraction
// into slices of `ktile` (the weight gradient; ktile = Kd otherwise).
enum { TRG_FWD_ACT = 0, TRG_FWD_LIN = 1, TRG_BWD_ACT = 2, TRG_BWD_LIN = 3, TRG_WGRAD = 4 };
struct TrGemm {
    const float* A; long long a_si, a_sk;
    const float* B; long long b_sk, b_sj;
    long long M; int N; long long Kd, ktile;
    int mode;                   // TRG_*
    const float* bias;          // FWD_*: [N]
    const float* dact;          // BWD_ACT: silu' of the layer in front, [M][ldo]
    float *out, *out2;          // FWD_ACT: silu(z), silu'(z); FWD_LIN: z; BWD_ACT: C o dact; BWD_LIN: C.  Row stride ldo
    long long ldo;
    float* part;                // WGRAD: slice z writes dW [M][Kin] at part[z part_stride + w_off ..]
    size_t part_stride, w_off; int Kin;
};
hipError_t launch_train_gemm(const TrGemm& g, int slices, hipStream_t st);

// rows idx[b] of src [n][m] into dst [B][m]; an index outside 0..n-1 reads row 0 (the host has refused it before)
hipError_t launch_train_gather(float* dst, const float* src, const long long* idx, long long n, long long B, int m, hipStream_t st);
// e0 [B][3] = (beta0, beta1, t)
hipError_t launch_train_embed_in(float* e0, const float* beta0, const float* beta1, const float* t, long long B, hipStream_t st);
// a0 [halves B][d + 2] = (xt row, t, embed) of either half
hipError_t launch_train_net_in(float* a0, const float* xt, const float* t, const float* emb, long long B, int halves, int d, hipStream_t st);
// gz [halves B][d] = (b - target) / B, target = (x1 - x0) +- gamma'(t) z (fp64, one rounding to fp32)
hipError_t launch_train_gout(float* gz, const VlossParams& p, hipStream_t st);
// ge [B] = sum_n w0 [n][K - 1] (gz0 [b][n] + gz0 [B + b][n]) in fp64, rounded once (one half: the first term alone); gz0 [halves B][H]
hipError_t launch_train_embed_gout(float* ge, const float* gz0, const float* w0, long long B, int halves, int H, int K, hipStream_t st);
// db [N] = the column sums of gz [rows][N] in fp64: 16 accumulators per column over the rows p, p + 16, .., added in order
hipError_t launch_train_bias(double* db, const float* gz, long long rows, int N, hipStream_t st);
// grad [n] = the slices of part in order where is_bias is 0 (part == NULL or a bias: grad as it stands), sq [n] = grad^2; entries below
// n_embed have tiles_e slices, the rest tiles_n
hipError_t launch_train_combine(double* grad, double* sq, const float* part, const unsigned char* is_bias, size_t part_stride, size_t n,
                                size_t n_embed, int tiles_e, int tiles_n, hipStream_t st);
struct TrAdam {
    double *w, *m, *v; float* w32; const double* grad; size_t n;
    const double* sumsq;        // [1] sum of grad^2
    const double* loss_sum;     // [1] sum of the loss rows, or NULL (ti_adw_train_apply)
    double B;
    double beta1, beta2, eps, weight_decay, max_norm;      // max_norm <= 0: no clipping
    const double* bias;         // [steps][2]: lr / (1 - beta1^k), sqrt(1 - beta2^k) for k = base + 1 + i
    long long* ctr;             // [2] n_applied, n_skipped
    long long base, base_skip;  // the counters when the call began: bias and log are indexed from them
    double* log;                // finish: the step's mean loss (NaN where skipped), or NULL
};
hipError_t launch_train_adam(const TrAdam& a, hipStream_t st);
hipError_t launch_train_finish(const TrAdam& a, hipStream_t st);
// w32 [n] = (float) w [n]
hipError_t launch_train_refresh(float* w32, const double* w, size_t n, hipStream_t st);

// the descriptor checks of the velocity loss (api_vloss.hip), shared with the trainer
int vloss_check(const ti_vloss_desc* d, const float* t, const float* z, int64_t B, int mem);

}  // namespace ti
