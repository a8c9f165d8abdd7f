// painn_train_graph_kernels.hip -- the molecule trainer on per-molecule graphs (include/ti_hip.h ti_painn_train_set_graphs): masked /
// ragged twins of the kernels of a training step that read the graph or run over a molecule's entries -- the velocity loss's
// interpolate, centre and reduce kernels as the trainer uses them (vloss_kernels.hip), and painn_train_kernels.hip's embedding inputs,
// edge embedding, message combine forward and reverse, output gradient and edge-type table -- with the kernel that expands the table
// rows of a call into what they read and the kernel that places the pad atoms.  Nine twins have no text of their own: a twin and its
// parent are one body (vloss_state_body.inc, painn_train_graph_body.inc), included here with the predicates on what is skipped and
// in the parent's unit with predicates that are `false` or nothing.  What is written out here has no parent (expand, pad) or another
// signature (the table, whose parent serves the atom table as well).
//
// One thread per (row, feature) like the parents; no atomics.  The dense products and column sums are the untouched kernels.
#include "painn_train_graph.hpp"
#include "vloss_device.hpp"

namespace ti {

namespace {

constexpr int PG_BLOCK = 256;
constexpr uint8_t PG_DEAD = 0x80;

unsigned pg_blocks(long long n) { return (unsigned)((n + PG_BLOCK - 1) / PG_BLOCK); }

__device__ __forceinline__ long long pg_index() { return (long long)blockIdx.x * PG_BLOCK + threadIdx.x; }

__global__ __launch_bounds__(PG_BLOCK) void ptg_expand_kernel(uint8_t* __restrict__ flag, int32_t* __restrict__ nat, const PtTable t,
                                                              const int32_t* __restrict__ etype, const PtGraph g, long long B)
{
    const long long i = pg_index();
    if (i >= B * g.E) return;
    const long long b = i / g.E;
    const int k = (int)(i - b * g.E);
    long long row = t.idx ? t.idx[b] : b;
    if (row < 0 || row >= t.n) row = 0;
    const int n = t.n_atoms[row], s = g.src[k], d = g.dst[k];
    const bool live = s < n && d < n && ((t.mask[row * g.A + d] >> (unsigned)s) & 1u) != 0u;
    const int type = t.ptype ? (int)t.ptype[(row * g.A + s) * g.A + d] : etype[k];
    flag[i] = (uint8_t)((type & 3) | (live ? 0 : PG_DEAD));
    if (k == 0) nat[b] = n;
}

// The twins: the bodies of vloss_kernels.hip's interpolate, centre and reduce kernels (ptg_interp_kernel, ptg_center_kernel,
// ptg_reduce_kernel) and of painn_train_kernels.hip's graph kernels (ptg_embed_in_kernel, ptg_edge_emb_kernel, ptg_msg_fwd_kernel,
// ptg_msg_bwd_edge_kernel, ptg_msg_bwd_node_kernel, ptg_gout_kernel), each with what a molecule of the call has of its own.  Both
// halves read molecule r % lv.B.  With a full table no predicate fires and lv.N = B A.
#define TI_TWIN_KERNEL(stem) ptg_##stem##_kernel
#define TI_TWIN_BLOCK PG_BLOCK
#define TI_TWIN_LIVE_PARAM , const PtLive lv
#define TI_MOL_ATOMS(b) lv.nat[b]
#define TI_MOL_ENTRIES(b) ((p.m / p.A) * lv.nat[b])
#define TI_PAD_ATOM(a, b) ((a) >= lv.nat[b])
#define TI_PAD_ENTRY(k, b) ((k) >= TI_MOL_ENTRIES(b))
#define TI_BATCH_ATOMS lv.N
#define TI_EDGE_TYPES_PARAM
#define TI_EDGE_TYPE(row) (lv.flag[((row) / g.E % lv.B) * g.E + (row) % g.E] & 3)
#define TI_EDGE_FLAGS(r) const uint8_t* fl = lv.flag + ((r) % lv.B) * g.E;
#define TI_EDGE_DEAD(k) (fl[k] & PG_DEAD)
#include "vloss_state_body.inc"
#include "painn_train_graph_body.inc"
#undef TI_TWIN_KERNEL
#undef TI_TWIN_BLOCK
#undef TI_TWIN_LIVE_PARAM
#undef TI_MOL_ATOMS
#undef TI_MOL_ENTRIES
#undef TI_PAD_ATOM
#undef TI_PAD_ENTRY
#undef TI_BATCH_ATOMS
#undef TI_EDGE_TYPES_PARAM
#undef TI_EDGE_TYPE
#undef TI_EDGE_FLAGS
#undef TI_EDGE_DEAD

// one thread per (half, molecule, atom)
__global__ __launch_bounds__(PG_BLOCK) void ptg_pad_kernel(float* __restrict__ xt, long long half, int halves, int A, const PtLive lv)
{
    const long long i = pg_index();
    if (i >= (long long)halves * lv.B * A) return;
    const long long r = i / A, hf = r / lv.B, b = r - hf * lv.B;
    const int a = (int)(i - r * A), nb = lv.nat[b];
    if (a < nb) return;
    float* x = xt + hf * half + b * 3 * A;
    x[3 * a] = x[0] + 100.0f * (float)(a - nb + 1); x[3 * a + 1] = x[1]; x[3 * a + 2] = x[2];
}

// pt_table_kernel with each molecule's own type per edge; a dead edge belongs to no table row
constexpr int PG_TAB_ACC = 16;
__global__ __launch_bounds__(64 * PG_TAB_ACC) void ptg_table_kernel(double* __restrict__ out, const float* __restrict__ g, long long ld, const PtGraph gr,
                                                                    const PtLive lv)
{
#pragma clang fp contract(off)
    __shared__ double sm[PG_TAB_ACC][64];
    const int F = gr.F, per = gr.E;
    const int c = threadIdx.x & 63, p = threadIdx.x >> 6, f = blockIdx.x * 64 + c, id = blockIdx.y;
    double s = 0.0;
    if (f < F)
        for (long long r = p; r < gr.R; r += PG_TAB_ACC) {
            const uint8_t* fl = lv.flag + (r % lv.B) * per;
            for (int a = 0; a < per; ++a)
                if ((int)fl[a] == id) s = s + (double)g[(r * per + a) * ld + f];
        }
    sm[p][c] = s;
    __syncthreads();
    if (p == 0 && f < F) {
        double t = 0.0;
        for (int q = 0; q < PG_TAB_ACC; ++q) t = t + sm[q][c];
        out[(size_t)id * F + f] = t;
    }
}

}  // namespace

#define PG_LAUNCH(kernel, count, ...) do { hipLaunchKernelGGL(kernel, dim3(pg_blocks(count)), dim3(PG_BLOCK), 0, st, __VA_ARGS__); return hipGetLastError(); } while (0)

hipError_t launch_ptg_expand(uint8_t* flag, int32_t* nat, const PtTable& t, const int32_t* etype, const PtGraph& g, long long B, hipStream_t st)
{
    PG_LAUNCH(ptg_expand_kernel, B * g.E, flag, nat, t, etype, g, B);
}
hipError_t launch_ptg_interp(const VlossParams& p, const PtLive& lv, hipStream_t st) { PG_LAUNCH(ptg_interp_kernel, p.B * p.m, p, lv); }
hipError_t launch_ptg_center(const VlossParams& p, const PtLive& lv, hipStream_t st)
{
    hipLaunchKernelGGL(ptg_center_kernel, dim3(pg_blocks(p.B * p.m), p.kind == TI_VLOSS_ONE_SIDED ? 1 : 2), dim3(PG_BLOCK), 0, st, p, lv);
    return hipGetLastError();
}
hipError_t launch_ptg_pad(float* xt, long long half, int halves, int A, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_pad_kernel, (long long)halves * lv.B * A, xt, half, halves, A, lv);
}
hipError_t launch_ptg_reduce(const VlossParams& p, const PtLive& lv, hipStream_t st) { PG_LAUNCH(ptg_reduce_kernel, p.B, p, lv); }
hipError_t launch_ptg_gout(float* gz, const VlossParams& p, const PtLive& lv, hipStream_t st) { PG_LAUNCH(ptg_gout_kernel, p.B * p.m, gz, p, lv); }
hipError_t launch_ptg_embed_in(float* s_in, const PtEmbedIn& e, const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_embed_in_kernel, g.R * g.A * e.nE * g.F, s_in, e, g, lv);
}
hipError_t launch_ptg_edge_emb(float* e0, const float* table, const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_edge_emb_kernel, g.R * g.E * g.F, e0, table, g, lv);
}
hipError_t launch_ptg_msg_fwd(float* s_out, float* v_out, const float* s, const float* v, const float* P, const float* Wd, const float* dir,
                              const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_msg_fwd_kernel, g.R * g.A * g.F, s_out, v_out, s, v, P, Wd, dir, g, lv);
}
hipError_t launch_ptg_msg_bwd_edge(float* gP, float* gWd, const float* gs, const float* gv, const float* ge, const float* v, const float* P,
                                   const float* Wd, const float* dir, const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_msg_bwd_edge_kernel, g.R * g.E * g.F, gP, gWd, gs, gv, ge, v, P, Wd, dir, g, lv);
}
hipError_t launch_ptg_msg_bwd_node(float* gs_out, float* gv_out, const float* gs, const float* gv, const float* gin_phi, const float* P,
                                   const float* Wd, const float* dir, const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_msg_bwd_node_kernel, g.R * g.A * g.F, gs_out, gv_out, gs, gv, gin_phi, P, Wd, dir, g, lv);
}
hipError_t launch_ptg_table(double* out, const float* g, long long ld, const PtGraph& gr, const PtLive& lv, hipStream_t st)
{
    hipLaunchKernelGGL(ptg_table_kernel, dim3((unsigned)((gr.F + 63) / 64), 4u), dim3(64 * PG_TAB_ACC), 0, st, out, g, ld, gr, lv);
    return hipGetLastError();
}

}  // namespace ti
