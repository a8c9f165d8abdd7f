// painn_train_graph.hpp -- private header of the molecule trainer on per-molecule graphs (include/ti_hip.h
// ti_painn_train_set_graphs): the launchers of painn_train_graph_kernels.hip, the masked / ragged twins of the kernels a call with a
// table in force cannot take as they stand.  Shared by that unit and api_painn_train.hip only.  A twin and its parent are one body
// (vloss_state_body.inc, painn_train_graph_body.inc); the notes at the launchers say what the twin's predicates do.  Everything else of such a call -- the
// geometry, the encodings, the products, LayerNorm, the update, the readout, the column sums -- is the kernels of a call without a
// table: they run over the dense layout, in which every row is finite and dead rows carry exact zeros where a sum would take them.
#pragma once
#include "painn_train.hpp"

namespace ti {

// The table of ti_painn_train_set_graphs on the device, and the rows of it a call reads: molecule b reads row idx[b] (NULL: row b).
struct PtTable {
    const int32_t* n_atoms;     // [n]
    const uint32_t* mask;       // [n][A], bit s of word d: s -> d
    const uint8_t* ptype;       // [n][A][A] at (s, d), or NULL: the template's types
    const long long* idx;       // [B] or NULL
    long long n;                // rows of the table; an index outside it reads row 0 (the host has refused it before)
};

// What the twins read of a call: flag [B][E], bit 7 set where template edge k of molecule b is DEAD (its bit is clear, or it touches a
// pad atom), bits 0..1 its type; nat [B] the atom counts; N = sum_b nat[b].  Molecule r of either half reads b = r % B.
struct PtLive {
    const uint8_t* flag; const int32_t* nat;
    long long B; double N;
};

// flag and nat of a call from the table rows it reads; one thread per (b, k), thread (b, 0) writes nat[b]
hipError_t launch_ptg_expand(uint8_t* flag, int32_t* nat, const PtTable& t, const int32_t* etype, const PtGraph& g, long long B, hipStream_t st);

// ---- the velocity loss's kernels as the trainer uses them (vloss_kernels.hip), over real entries
// interp: a pad entry draws nothing, z = 0 there, raw = +0.0 (BATCH / MOLECULE; launch_vloss_colsum then adds the pads as +0.0), xt is
// left to launch_ptg_pad.  center: BATCH divides the column sums by N, MOLECULE sums the nat[b] real atoms in order and divides by nat[b].
hipError_t launch_ptg_interp(const VlossParams& p, const PtLive& lv, hipStream_t st);
hipError_t launch_ptg_center(const VlossParams& p, const PtLive& lv, hipStream_t st);
// xt of pad atom a of molecule r = xt[r][0] + (100 (a - nat + 1), 0, 0), both halves; behind interp (NONE) or center
hipError_t launch_ptg_pad(float* xt, long long half, int halves, int A, const PtLive& lv, hipStream_t st);
// loss [B]: vloss_reduce over the 3 nat[b] real entries of a molecule in order
hipError_t launch_ptg_reduce(const VlossParams& p, const PtLive& lv, hipStream_t st);
// gz = (b - target) / N on real entries, +0 on pads
hipError_t launch_ptg_gout(float* gz, const VlossParams& p, const PtLive& lv, hipStream_t st);

// ---- painn_train_kernels.hip's kernels that read the graph
// cond of a pad atom is 0
hipError_t launch_ptg_embed_in(float* s_in, const PtEmbedIn& e, const PtGraph& g, const PtLive& lv, hipStream_t st);
// e0 = table[type of (b, k)]
hipError_t launch_ptg_edge_emb(float* e0, const float* table, const PtGraph& g, const PtLive& lv, hipStream_t st);
// the per-node sums skip dead edges
hipError_t launch_ptg_msg_fwd(float* s_out, float* v_out, const float* s, const float* v, const float* P, const float* Wd, const float* dir,
                              const PtGraph& g, const PtLive& lv, hipStream_t st);
// gP, gWd rows of dead edges = +0
hipError_t launch_ptg_msg_bwd_edge(float* gP, float* gWd, const float* gs, const float* gv, const float* ge, const float* v, const float* P,
                                   const float* Wd, const float* dir, const PtGraph& g, const PtLive& lv, hipStream_t st);
hipError_t launch_ptg_msg_bwd_node(float* gs_out, float* gv_out, const float* gs, const float* gv, const float* gin_phi, const float* P,
                                   const float* Wd, const float* dir, const PtGraph& g, const PtLive& lv, hipStream_t st);
// the edge-type table's gradient: out [4][F] = the sums of g [R E][ld] over the live edge rows whose own type is the table row, in the
// order of launch_ptrain_table
hipError_t launch_ptg_table(double* out, const float* g, long long ld, const PtGraph& gr, const PtLive& lv, hipStream_t st);

}  // namespace ti
