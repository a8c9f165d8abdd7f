// painn_train.hpp -- private header of the molecule trainer (include/ti_hip.h ti_painn_trainer_create .. ti_painn_train_workspace_bytes):
// the launchers of painn_train_kernels.hip.  Shared by painn_train_kernels.hip and api_painn_train.hip, and through
// painn_train_graph.hpp by painn_train_graph_kernels.hip, which is why the positional encoding both kernel units evaluate is stated
// here.  The matrix products, the combine of the weight-gradient slices and clip + Adam are the adw trainer's (adw_train.hpp).
//
// Rows: a call evaluates R = halves B molecules, molecule r = half B + b.  Node row n = r A + a, edge row r E + k (k the template
// edge).  Per-node vectors v lie as [n][3][F], so that U v and V v are products over 3 R A rows of F.
#pragma once
#include "adw_train.hpp"

namespace ti {

// rows per slice of a weight-gradient contraction: fixed, so a gradient does not depend on the launch.  Each slice is one fp32 fmaf
// chain per entry, the slices are added in fp64.
constexpr int PTRAIN_SLICE = 2048;
inline long long ptrain_slices(long long rows) { return (rows + PTRAIN_SLICE - 1) / PTRAIN_SLICE; }

// feature f of PositionalEncoder: cos, sin interleaved per k = f / 2 + 1
constexpr float PT_PI = 3.14159265358979323846f;
__device__ __forceinline__ float pt_posenc(float x_over_len, int f)
{
    const float arg = (x_over_len * (float)(f / 2 + 1)) * PT_PI;
    return (f & 1) ? sinf(arg) : cosf(arg);
}

struct PtGraph {
    const int32_t *src, *dst;   // [E] the template
    int A, E, F;
    long long R;                // molecules of the call, both halves
};

// dir [R E][3] = r / (1 + d), dist [R E] = d, r = x[src] - x[dst]; x [R][A][3]
hipError_t launch_ptrain_geom(float* dir, float* dist, const float* x, const PtGraph& g, hipStream_t st);
// enc [R E][F] = PositionalEncoder(d / length_scale)
hipError_t launch_ptrain_enc(float* enc, const float* dist, float length_scale, const PtGraph& g, hipStream_t st);
// s_in [R A][nE F] = [atom embedding | enc(T0) | enc(T1) | enc(t)] (ambient; the latent variants have one or no temperature);
// cond [B][A][ncond] and t [B] are shared by the halves
struct PtEmbedIn {
    const float *atom_emb, *cond, *t; const int32_t* atom_ids;
    int ncond, nE; long long B;
    float temp_length, time_length, temp_mean, temp_range;
};
hipError_t launch_ptrain_embed_in(float* s_in, const PtEmbedIn& e, const PtGraph& g, hipStream_t st);
// e0 [R E][F] = table[etype[k]]
hipError_t launch_ptrain_edge_emb(float* e0, const float* table, const int32_t* etype, const PtGraph& g, hipStream_t st);
// y [rows][F] = silu(LayerNorm(z) gamma + beta), eps 1e-5, biased variance
hipError_t launch_ptrain_ln_fwd(float* y, const float* z, const float* gamma, const float* beta, long long rows, int F, hipStream_t st);
// from gy = dL/dy: gz = dL/dz, gu = dL/d(LayerNorm output) (its column sum is the gradient of beta), guxh = gu xhat (gamma's)
hipError_t launch_ptrain_ln_bwd(float* gz, float* gu, float* guxh, const float* gy, const float* z, const float* gamma, const float* beta,
                                long long rows, int F, hipStream_t st);
// phi_in [R E][2F] = [s[src] | e]
hipError_t launch_ptrain_phi_in(float* phi_in, const float* s, const float* e, const PtGraph& g, hipStream_t st);
// the message combine of a layer: h = P o Wd [R E][5F] in chunks (gates, scale, ds, de, cross gates);
// s_out = s + sum ds, v_out = v + sum (scale dir + gates v[src] + cross (dir x v[dst])) over a node's incoming edges in template order
hipError_t launch_ptrain_msg_fwd(float* s_out, float* v_out, const float* s, const float* v, const float* P, const float* Wd, const float* dir,
                                 const PtGraph& g, hipStream_t st);
// e_out = e + de
hipError_t launch_ptrain_e_fwd(float* e_out, const float* e, const float* P, const float* Wd, const PtGraph& g, hipStream_t st);
// gP, gWd [R E][5F] from the gradients at the layer's outputs gs, gv (nodes) and ge (edges; NULL: zero, the last layer)
hipError_t launch_ptrain_msg_bwd_edge(float* gP, float* gWd, const float* gs, const float* gv, const float* ge, const float* v, const float* P,
                                      const float* Wd, const float* dir, const PtGraph& g, hipStream_t st);
// gs_out = gs + sum over outgoing edges of gin_phi[:, :F]; gv_out = gv + sum over outgoing edges gates gv[dst] + sum over incoming
// edges cross (gv x dir); ge_out = ge + gin_phi[:, F:]
hipError_t launch_ptrain_msg_bwd_node(float* gs_out, float* gv_out, const float* gs, const float* gv, const float* gin_phi, const float* P,
                                      const float* Wd, const float* dir, const PtGraph& g, hipStream_t st);
hipError_t launch_ptrain_e_bwd(float* ge_out, const float* ge, const float* gin_phi, const PtGraph& g, hipStream_t st);
// up_in [R A][2F] = [ ||vv|| | s ]
hipError_t launch_ptrain_upd_in(float* up_in, const float* vv, const float* s, const PtGraph& g, hipStream_t st);
// v_out = v + uv g, s_out = s + n^2 q + a; gqa [R A][3F]
hipError_t launch_ptrain_upd_apply(float* s_out, float* v_out, const float* s, const float* v, const float* uv, const float* up_in, const float* gqa,
                                   const PtGraph& g, hipStream_t st);
// gout [R A][3F] = (sum_c gv uv, gs n^2, gs), guv = gv g
hipError_t launch_ptrain_upd_bwd_a(float* gout, float* guv, const float* gs, const float* gv, const float* uv, const float* up_in, const float* gqa,
                                   const PtGraph& g, hipStream_t st);
// gvv = (gs 2 n q + gin[:, :F]) vv / n (0 where n = 0), gs_out = gs + gin[:, F:]
hipError_t launch_ptrain_upd_bwd_b(float* gvv, float* gs_out, const float* gs, const float* gin, const float* vv, const float* up_in, const float* gqa,
                                   const PtGraph& g, hipStream_t st);
// out [n] = a + b + c
hipError_t launch_ptrain_add3(float* out, const float* a, const float* b, const float* c, long long n, hipStream_t st);
// b [R A][3] = Vv gate, gate = ro[:, 1]
hipError_t launch_ptrain_readout(float* b, const float* Vv, const float* ro, long long nodes, hipStream_t st);
// gz [halves][B][m] = (b - target) / (B A) in fp64, rounded once; target = (x1 - x0) +- gamma'(t) z
hipError_t launch_ptrain_gout(float* gz, const VlossParams& p, hipStream_t st);
// gro [R A][2] = (0, sum_c gb Vv), gVv [R A][3] = gb gate, gv [R A][3][F] = gVv Vr
hipError_t launch_ptrain_readout_bwd(float* gro, float* gVv, float* gv, const float* gb, const float* Vv, const float* ro, const float* Vr,
                                     const PtGraph& g, hipStream_t st);
// out [N] = the column sums of gz [rows][N] in fp64, in tiles of PTRAIN_SLICE rows: within a tile accumulator p of 16 adds the tile's
// rows p, p + 16, .. in order from +0.0 and the accumulators are added in order (partial [tiles][N]); then the tiles in order
hipError_t launch_ptrain_colsum(double* out, double* partial, const float* gz, long long rows, int N, hipStream_t st);
// out [n_ids][F] = the sums of g [R per][ld] (its first F columns) over the rows whose template id is the table row, in fp64:
// accumulator p of 16 adds molecules p, p + 16, .. in order (a molecule's rows in template order), then the accumulators in order
hipError_t launch_ptrain_table(double* out, const float* g, long long ld, const int32_t* ids, int per, int n_ids, long long R, int F, hipStream_t st);

}  // namespace ti
