// painn_train_kernels.hip -- training cPaiNN on the velocity loss (include/ti_hip.h ti_painn_train_*): everything of the forward and
// the reverse pass that is not a matrix product.  The fused drift kernels keep nothing in HBM; this forward pass writes every
// intermediate the reverse pass reads.  The products, the fp64 column sums and the optimiser are the adw trainer's kernels
// (adw_train_kernels.hip), called through their launchers as they stand.
//
// One thread per (row, feature) throughout, except LayerNorm (one wave per row, a fixed shuffle tree) and the table gradient
// and the column sums (the accumulator scheme of adwtr_bias_kernel, per tile of rows).  No atomics: a per-node sum walks the template's edges in order.
// The six kernels that per-molecule graphs change have their bodies in painn_train_graph_body.inc, which painn_train_graph_kernels.hip
// includes as well; gamma'(t) of the output gradient is the velocity loss's (vloss_device.hpp).
#include "painn_train.hpp"
#include "vloss_device.hpp"

namespace ti {

namespace {

constexpr int PT_BLOCK = 256;

unsigned pt_blocks(long long n) { return (unsigned)((n + PT_BLOCK - 1) / PT_BLOCK); }

__device__ __forceinline__ long long pt_index() { return (long long)blockIdx.x * PT_BLOCK + threadIdx.x; }

// The kernels that read the graph or run over a molecule's entries: pt_embed_in_kernel, pt_edge_emb_kernel, pt_msg_fwd_kernel,
// pt_msg_bwd_edge_kernel, pt_msg_bwd_node_kernel and pt_gout_kernel.  Every molecule is the whole template here: no pads, no dead
// edges, the template's edge types; painn_train_graph_kernels.hip takes the same text with each molecule's own
#define TI_TWIN_KERNEL(stem) pt_##stem##_kernel
#define TI_TWIN_BLOCK PT_BLOCK
#define TI_TWIN_LIVE_PARAM
#define TI_PAD_ATOM(a, b) false
#define TI_PAD_ENTRY(k, b) false
#define TI_BATCH_ATOMS (double)(p.B * p.A)
#define TI_EDGE_TYPES_PARAM const int32_t* __restrict__ etype,
#define TI_EDGE_TYPE(row) etype[(row) % g.E]
#define TI_EDGE_FLAGS(r)
#define TI_EDGE_DEAD(k) false
#include "painn_train_graph_body.inc"
#undef TI_TWIN_KERNEL
#undef TI_TWIN_BLOCK
#undef TI_TWIN_LIVE_PARAM
#undef TI_PAD_ATOM
#undef TI_PAD_ENTRY
#undef TI_BATCH_ATOMS
#undef TI_EDGE_TYPES_PARAM
#undef TI_EDGE_TYPE
#undef TI_EDGE_FLAGS
#undef TI_EDGE_DEAD

__global__ __launch_bounds__(PT_BLOCK) void pt_geom_kernel(float* __restrict__ dir, float* __restrict__ dist, const float* __restrict__ x, const PtGraph g)
{
    const long long i = pt_index();
    if (i >= g.R * g.E) return;
    const long long r = i / g.E;
    const int k = (int)(i - r * g.E);
    const float* xs = x + (r * g.A + g.src[k]) * 3;
    const float* xd = x + (r * g.A + g.dst[k]) * 3;
    const float rx = xs[0] - xd[0], ry = xs[1] - xd[1], rz = xs[2] - xd[2];
    const float d = sqrtf(rx * rx + ry * ry + rz * rz), den = 1.0f + d;
    dir[3 * i] = rx / den; dir[3 * i + 1] = ry / den; dir[3 * i + 2] = rz / den;
    dist[i] = d;
}

__global__ __launch_bounds__(PT_BLOCK) void pt_enc_kernel(float* __restrict__ enc, const float* __restrict__ dist, float length_scale, const PtGraph g)
{
    const long long i = pt_index();
    if (i >= g.R * g.E * g.F) return;
    const long long row = i / g.F;
    enc[i] = pt_posenc(dist[row] / length_scale, (int)(i - row * g.F));
}

__device__ __forceinline__ float pt_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// LayerNorm of a row held four entries a lane: xhat and rstd
__device__ __forceinline__ float pt_ln_stats(float (&x)[4], const float* __restrict__ z, int F, int lane)
{
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int f = lane + 64 * j; x[j] = f < F ? z[f] : 0.f; s += x[j]; }
    const float mean = pt_wave_sum(s) / (float)F;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int f = lane + 64 * j; x[j] = f < F ? x[j] - mean : 0.f; q += x[j] * x[j]; }
    const float rstd = 1.0f / sqrtf(pt_wave_sum(q) / (float)F + 1e-5f);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] *= rstd;
    return rstd;
}

__global__ __launch_bounds__(PT_BLOCK) void pt_ln_fwd_kernel(float* __restrict__ y, const float* __restrict__ z, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, long long rows, int F)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (PT_BLOCK / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                       // the whole wave
    float xh[4];
    pt_ln_stats(xh, z + row * F, F, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = lane + 64 * j;
        if (f >= F) continue;
        const float u = xh[j] * gamma[f] + beta[f];
        y[row * F + f] = u / (1.0f + expf(-u));
    }
}

__global__ __launch_bounds__(PT_BLOCK) void pt_ln_bwd_kernel(float* __restrict__ gz, float* __restrict__ gu, float* __restrict__ guxh,
                                                             const float* __restrict__ gy, const float* __restrict__ z, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, long long rows, int F)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (PT_BLOCK / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    float xh[4], gx[4];
    const float rstd = pt_ln_stats(xh, z + row * F, F, lane);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = lane + 64 * j;
        gx[j] = 0.f;
        if (f >= F) continue;
        const float u = xh[j] * gamma[f] + beta[f], sg = 1.0f / (1.0f + expf(-u)), y = u * sg;
        const float g = gy[row * F + f] * fmaf(y, 1.0f - sg, sg);
        gu[row * F + f] = g;
        guxh[row * F + f] = g * xh[j];
        gx[j] = g * gamma[f];
        m1 += gx[j]; m2 += gx[j] * xh[j];
    }
    m1 = pt_wave_sum(m1) / (float)F; m2 = pt_wave_sum(m2) / (float)F;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = lane + 64 * j;
        if (f < F) gz[row * F + f] = rstd * (gx[j] - m1 - xh[j] * m2);
    }
}

__global__ __launch_bounds__(PT_BLOCK) void pt_phi_in_kernel(float* __restrict__ phi_in, const float* __restrict__ s, const float* __restrict__ e, const PtGraph g)
{
    const int K = 2 * g.F;
    const long long i = pt_index();
    if (i >= g.R * g.E * K) return;
    const long long row = i / K, r = row / g.E;
    const int j = (int)(i - row * K), k = (int)(row - r * g.E);
    phi_in[i] = j < g.F ? s[(r * g.A + g.src[k]) * g.F + j] : e[row * g.F + (j - g.F)];
}

__global__ __launch_bounds__(PT_BLOCK) void pt_e_fwd_kernel(float* __restrict__ e_out, const float* __restrict__ e, const float* __restrict__ P,
                                                            const float* __restrict__ Wd, const PtGraph g)
{
    const long long i = pt_index();
    if (i >= g.R * g.E * g.F) return;
    const long long row = i / g.F, o = row * 5 * g.F + 3 * g.F + (i - row * g.F);
    e_out[i] = e[i] + P[o] * Wd[o];
}

__global__ __launch_bounds__(PT_BLOCK) void pt_e_bwd_kernel(float* __restrict__ ge_out, const float* __restrict__ ge, const float* __restrict__ gin_phi,
                                                            const PtGraph g)
{
    const long long i = pt_index();
    if (i >= g.R * g.E * g.F) return;
    const long long row = i / g.F;
    const float b = gin_phi[row * 2 * g.F + g.F + (i - row * g.F)];
    ge_out[i] = ge ? ge[i] + b : b;
}

__global__ __launch_bounds__(PT_BLOCK) void pt_upd_in_kernel(float* __restrict__ up_in, const float* __restrict__ vv, const float* __restrict__ s, const PtGraph g)
{
    const int F = g.F;
    const long long i = pt_index();
    if (i >= g.R * g.A * F) return;
    const long long n = i / F;
    const int f = (int)(i - n * F);
    const float a = vv[(n * 3) * F + f], b = vv[(n * 3 + 1) * F + f], c = vv[(n * 3 + 2) * F + f];
    up_in[n * 2 * F + f] = sqrtf(a * a + b * b + c * c);
    up_in[n * 2 * F + F + f] = s[i];
}

__global__ __launch_bounds__(PT_BLOCK) void pt_upd_apply_kernel(float* __restrict__ s_out, float* __restrict__ v_out, const float* __restrict__ s,
                                                                const float* __restrict__ v, const float* __restrict__ uv, const float* __restrict__ up_in,
                                                                const float* __restrict__ gqa, const PtGraph g)
{
    const int F = g.F;
    const long long i = pt_index();
    if (i >= g.R * g.A * F) return;
    const long long n = i / F;
    const int f = (int)(i - n * F);
    const float gg = gqa[n * 3 * F + f], q = gqa[n * 3 * F + F + f], a = gqa[n * 3 * F + 2 * F + f], nn = up_in[n * 2 * F + f];
#pragma unroll
    for (int c = 0; c < 3; ++c) v_out[(n * 3 + c) * F + f] = v[(n * 3 + c) * F + f] + uv[(n * 3 + c) * F + f] * gg;
    s_out[i] = s[i] + (nn * nn) * q + a;
}

__global__ __launch_bounds__(PT_BLOCK) void pt_upd_bwd_a_kernel(float* __restrict__ gout, float* __restrict__ guv, const float* __restrict__ gs,
                                                                const float* __restrict__ gv, const float* __restrict__ uv, const float* __restrict__ up_in,
                                                                const float* __restrict__ gqa, const PtGraph g)
{
    const int F = g.F;
    const long long i = pt_index();
    if (i >= g.R * g.A * F) return;
    const long long n = i / F;
    const int f = (int)(i - n * F);
    const float gg = gqa[n * 3 * F + f], nn = up_in[n * 2 * F + f], gsv = gs[i];
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float gvc = gv[(n * 3 + c) * F + f];
        acc += gvc * uv[(n * 3 + c) * F + f];
        guv[(n * 3 + c) * F + f] = gvc * gg;
    }
    gout[n * 3 * F + f] = acc;
    gout[n * 3 * F + F + f] = gsv * (nn * nn);
    gout[n * 3 * F + 2 * F + f] = gsv;
}

__global__ __launch_bounds__(PT_BLOCK) void pt_upd_bwd_b_kernel(float* __restrict__ gvv, float* __restrict__ gs_out, const float* __restrict__ gs,
                                                                const float* __restrict__ gin, const float* __restrict__ vv, const float* __restrict__ up_in,
                                                                const float* __restrict__ gqa, const PtGraph g)
{
    const int F = g.F;
    const long long i = pt_index();
    if (i >= g.R * g.A * F) return;
    const long long n = i / F;
    const int f = (int)(i - n * F);
    const float q = gqa[n * 3 * F + F + f], nn = up_in[n * 2 * F + f], gsv = gs[i];
    const float gn = gsv * (2.0f * nn * q) + gin[n * 2 * F + f];
#pragma unroll
    for (int c = 0; c < 3; ++c) gvv[(n * 3 + c) * F + f] = nn > 0.0f ? gn * (vv[(n * 3 + c) * F + f] / nn) : 0.0f;      // torch: 0 at the origin
    gs_out[i] = gsv + gin[n * 2 * F + F + f];
}

__global__ __launch_bounds__(PT_BLOCK) void pt_add3_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ c, long long n)
{
    const long long i = pt_index();
    if (i < n) out[i] = a[i] + b[i] + c[i];
}

__global__ __launch_bounds__(PT_BLOCK) void pt_readout_kernel(float* __restrict__ b, const float* __restrict__ Vv, const float* __restrict__ ro, long long nodes)
{
    const long long i = pt_index();
    if (i < nodes * 3) b[i] = Vv[i] * ro[(i / 3) * 2 + 1];
}

__global__ __launch_bounds__(PT_BLOCK) void pt_readout_bwd_kernel(float* __restrict__ gro, float* __restrict__ gVv, float* __restrict__ gv,
                                                                  const float* __restrict__ gb, const float* __restrict__ Vv, const float* __restrict__ ro,
                                                                  const float* __restrict__ Vr, const PtGraph g)
{
    const int F = g.F;
    const long long i = pt_index();
    if (i >= g.R * g.A * F) return;
    const long long n = i / F;
    const int f = (int)(i - n * F);
    const float gate = ro[n * 2 + 1], vr = Vr[f];
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float gbc = gb[n * 3 + c];
        acc += gbc * Vv[n * 3 + c];
        gv[(n * 3 + c) * F + f] = (gbc * gate) * vr;
        if (f == 0) gVv[n * 3 + c] = gbc * gate;
    }
    if (f == 0) { gro[n * 2] = 0.0f; gro[n * 2 + 1] = acc; }
}

// The column sums of a layer's g (bias and LayerNorm gradients): adwtr_bias_kernel's accumulator scheme per tile of PTRAIN_SLICE rows,
// so that the rows of a large batch are spread over many blocks; the tiles are added in order by a second launch.  grid (N / 64, tiles)
constexpr int PT_TAB_ACC = 16;
__global__ __launch_bounds__(64 * PT_TAB_ACC) void pt_colsum_tile_kernel(double* __restrict__ partial, const float* __restrict__ gz, long long rows, int N)
{
#pragma clang fp contract(off)
    __shared__ double sm[PT_TAB_ACC][64];
    const int c = threadIdx.x & 63, p = threadIdx.x >> 6, n = blockIdx.x * 64 + c;
    const long long r0 = (long long)blockIdx.y * PTRAIN_SLICE, r1 = min(rows, r0 + PTRAIN_SLICE);
    double s = 0.0;
    if (n < N)
        for (long long r = r0 + p; r < r1; r += PT_TAB_ACC) s = s + (double)gz[r * N + n];
    sm[p][c] = s;
    __syncthreads();
    if (p == 0 && n < N) {
        double t = 0.0;
        for (int q = 0; q < PT_TAB_ACC; ++q) t = t + sm[q][c];
        partial[(size_t)blockIdx.y * N + n] = t;
    }
}

__global__ __launch_bounds__(PT_BLOCK) void pt_colsum_combine_kernel(double* __restrict__ out, const double* __restrict__ partial, int tiles, int N)
{
#pragma clang fp contract(off)
    const long long n = pt_index();
    if (n >= N) return;
    double t = 0.0;
    for (int z = 0; z < tiles; ++z) t = t + partial[(size_t)z * N + n];
    out[n] = t;
}

__global__ __launch_bounds__(64 * PT_TAB_ACC) void pt_table_kernel(double* __restrict__ out, const float* __restrict__ g, long long ld,
                                                                   const int32_t* __restrict__ ids, int per, long long R, int F)
{
#pragma clang fp contract(off)
    __shared__ double sm[PT_TAB_ACC][64];
    const int c = threadIdx.x & 63, p = threadIdx.x >> 6, f = blockIdx.x * 64 + c, id = blockIdx.y;
    double s = 0.0;
    if (f < F)
        for (long long r = p; r < R; r += PT_TAB_ACC)
            for (int a = 0; a < per; ++a)
                if (ids[a] == id) s = s + (double)g[(r * per + a) * ld + f];
    sm[p][c] = s;
    __syncthreads();
    if (p == 0 && f < F) {
        double t = 0.0;
        for (int q = 0; q < PT_TAB_ACC; ++q) t = t + sm[q][c];
        out[(size_t)id * F + f] = t;
    }
}

}  // namespace

#define PT_LAUNCH(kernel, count, ...) do { hipLaunchKernelGGL(kernel, dim3(pt_blocks(count)), dim3(PT_BLOCK), 0, st, __VA_ARGS__); return hipGetLastError(); } while (0)

hipError_t launch_ptrain_geom(float* dir, float* dist, const float* x, const PtGraph& g, hipStream_t st) { PT_LAUNCH(pt_geom_kernel, g.R * g.E, dir, dist, x, g); }
hipError_t launch_ptrain_enc(float* enc, const float* dist, float length_scale, const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_enc_kernel, g.R * g.E * g.F, enc, dist, length_scale, g);
}
hipError_t launch_ptrain_embed_in(float* s_in, const PtEmbedIn& e, const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_embed_in_kernel, g.R * g.A * e.nE * g.F, s_in, e, g);
}
hipError_t launch_ptrain_edge_emb(float* e0, const float* table, const int32_t* etype, const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_edge_emb_kernel, g.R * g.E * g.F, e0, table, etype, g);
}
hipError_t launch_ptrain_ln_fwd(float* y, const float* z, const float* gamma, const float* beta, long long rows, int F, hipStream_t st)
{
    PT_LAUNCH(pt_ln_fwd_kernel, rows * 64, y, z, gamma, beta, rows, F);
}
hipError_t launch_ptrain_ln_bwd(float* gz, float* gu, float* guxh, const float* gy, const float* z, const float* gamma, const float* beta,
                                long long rows, int F, hipStream_t st)
{
    PT_LAUNCH(pt_ln_bwd_kernel, rows * 64, gz, gu, guxh, gy, z, gamma, beta, rows, F);
}
hipError_t launch_ptrain_phi_in(float* phi_in, const float* s, const float* e, const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_phi_in_kernel, g.R * g.E * 2 * g.F, phi_in, s, e, g);
}
hipError_t launch_ptrain_msg_fwd(float* s_out, float* v_out, const float* s, const float* v, const float* P, const float* Wd, const float* dir,
                                 const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_msg_fwd_kernel, g.R * g.A * g.F, s_out, v_out, s, v, P, Wd, dir, g);
}
hipError_t launch_ptrain_e_fwd(float* e_out, const float* e, const float* P, const float* Wd, const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_e_fwd_kernel, g.R * g.E * g.F, e_out, e, P, Wd, g);
}
hipError_t launch_ptrain_msg_bwd_edge(float* gP, float* gWd, const float* gs, const float* gv, const float* ge, const float* v, const float* P,
                                      const float* Wd, const float* dir, const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_msg_bwd_edge_kernel, g.R * g.E * g.F, gP, gWd, gs, gv, ge, v, P, Wd, dir, g);
}
hipError_t launch_ptrain_msg_bwd_node(float* gs_out, float* gv_out, const float* gs, const float* gv, const float* gin_phi, const float* P,
                                      const float* Wd, const float* dir, const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_msg_bwd_node_kernel, g.R * g.A * g.F, gs_out, gv_out, gs, gv, gin_phi, P, Wd, dir, g);
}
hipError_t launch_ptrain_e_bwd(float* ge_out, const float* ge, const float* gin_phi, const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_e_bwd_kernel, g.R * g.E * g.F, ge_out, ge, gin_phi, g);
}
hipError_t launch_ptrain_upd_in(float* up_in, const float* vv, const float* s, const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_upd_in_kernel, g.R * g.A * g.F, up_in, vv, s, g);
}
hipError_t launch_ptrain_upd_apply(float* s_out, float* v_out, const float* s, const float* v, const float* uv, const float* up_in, const float* gqa,
                                   const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_upd_apply_kernel, g.R * g.A * g.F, s_out, v_out, s, v, uv, up_in, gqa, g);
}
hipError_t launch_ptrain_upd_bwd_a(float* gout, float* guv, const float* gs, const float* gv, const float* uv, const float* up_in, const float* gqa,
                                   const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_upd_bwd_a_kernel, g.R * g.A * g.F, gout, guv, gs, gv, uv, up_in, gqa, g);
}
hipError_t launch_ptrain_upd_bwd_b(float* gvv, float* gs_out, const float* gs, const float* gin, const float* vv, const float* up_in, const float* gqa,
                                   const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_upd_bwd_b_kernel, g.R * g.A * g.F, gvv, gs_out, gs, gin, vv, up_in, gqa, g);
}
hipError_t launch_ptrain_add3(float* out, const float* a, const float* b, const float* c, long long n, hipStream_t st)
{
    PT_LAUNCH(pt_add3_kernel, n, out, a, b, c, n);
}
hipError_t launch_ptrain_readout(float* b, const float* Vv, const float* ro, long long nodes, hipStream_t st)
{
    PT_LAUNCH(pt_readout_kernel, nodes * 3, b, Vv, ro, nodes);
}
hipError_t launch_ptrain_gout(float* gz, const VlossParams& p, hipStream_t st) { PT_LAUNCH(pt_gout_kernel, p.B * p.m, gz, p); }
hipError_t launch_ptrain_readout_bwd(float* gro, float* gVv, float* gv, const float* gb, const float* Vv, const float* ro, const float* Vr,
                                     const PtGraph& g, hipStream_t st)
{
    PT_LAUNCH(pt_readout_bwd_kernel, g.R * g.A * g.F, gro, gVv, gv, gb, Vv, ro, Vr, g);
}
hipError_t launch_ptrain_colsum(double* out, double* partial, const float* gz, long long rows, int N, hipStream_t st)
{
    const int tiles = (int)ptrain_slices(rows);
    hipLaunchKernelGGL(pt_colsum_tile_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)tiles), dim3(64 * PT_TAB_ACC), 0, st, partial, gz, rows, N);
    hipLaunchKernelGGL(pt_colsum_combine_kernel, dim3(pt_blocks(N)), dim3(PT_BLOCK), 0, st, out, partial, tiles, N);
    return hipGetLastError();
}
hipError_t launch_ptrain_table(double* out, const float* g, long long ld, const int32_t* ids, int per, int n_ids, long long R, int F, hipStream_t st)
{
    hipLaunchKernelGGL(pt_table_kernel, dim3((unsigned)((F + 63) / 64), (unsigned)n_ids), dim3(64 * PT_TAB_ACC), 0, st, out, g, ld, ids, per, R, F);
    return hipGetLastError();
}

}  // namespace ti
