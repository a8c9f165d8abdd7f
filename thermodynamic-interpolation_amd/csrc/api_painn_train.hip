// api_painn_train.hip -- the molecule trainer of the C ABI (include/ti_hip.h ti_painn_trainer_create .. ti_painn_train_noise):
// the checks, the workspace plan, and the launch sequence of a training step -- interpolate and centre (vloss_kernels.hip), a forward
// pass through cPaiNN that keeps every intermediate, loss rows (the velocity loss's own reduce kernel), the reverse pass, the fp64
// combine of every parameter block, clip + Adam (adw_train_kernels.hip).  The products are the adw trainer's kernel; the column sums are
// painn_train_kernels.hip's tiled twin of its bias kernel.  A step is enqueued on the handle's stream without a host
// synchronisation: whether it is skipped is decided by the optimiser kernel from the two batch-wide sums in device memory.
// ti_painn_train_steps enqueues many such steps on resident sets (painn_steps_kernels.hip gathers each minibatch, painn_noise_kernels.hip
// draws the latent base samples) and synchronises once.
// The optimiser shell -- master state, counters, clip + Adam, the state entry points, index handling -- is train_optim.hpp's, shared
// with api_adw_train.hip.
// With a table of per-molecule graphs in force (ti_painn_train_set_graphs) a call expands the rows it reads into per-call flags and
// takes painn_train_graph_kernels.hip's twins where a kernel reads the graph or a molecule's entries; every other launch is the same.
#include "train_optim.hpp"
#include "painn_steps.hpp"
#include "painn_train_graph.hpp"

namespace {

constexpr int RED_COLSUM = 2;      // slots of PainnTrainState::red behind RED_LOSS and RED_SUMSQ (the column sums take 6)

struct Rec { size_t z1, y1, z2, y2; };       // what an MLP keeps: the two pre-LayerNorm rows and the two activations
struct LayerAct { size_t s_in, v_in, e_in, phi_in, P, Wd, s_m, v_m, uv, vv, up_in, gqa, s_out, v_out; Rec phi, w, upd; };

// the arena of one call (floats), laid out by plan(): the forward pass's records, then the reverse pass's buffers
struct Plan {
    size_t xt, z, dir, dist, enc, s_in0; Rec emb; std::vector<LayerAct> layers; Rec ro; size_t ro_out, Vv, bout;
    size_t gb, gro, gVv, gs[2], gv[2], ge[2], gP, gWd, gin_phi, t_gy, t_gz, t_gu, t_gx, gup, gin_up, guv, gvv, tmp1, tmp2, gin_emb;
    size_t total = 0;
};

struct PainnTrainState : Optim {                 // is_bias: 1 at the biases, LayerNorm entries and tables; red holds 8 (RED_COLSUM)
    ti_painn_desc d{};
    unsigned long long max_workspace_bytes = 0;  // the train descriptor's
    int nE = 0, ncond = 0;
    size_t edge_emb = 0, atom_emb = 0, Vr = 0, max_block = 0;
    MlpOff embed{}, readout{}; std::vector<MlpOff> phi, filt, upd; std::vector<size_t> U, V;      // filt: the filter MLP (w of ti_handle)
    DevBuf<double> loss, raw, colpart;           // colpart: the tile partials of a column sum
    DevBuf<float> part, arena, sx0, sx1, sc, tin, zin, t;
    DevBuf<int32_t> src, dst, etype, atom_ids;
    // ti_painn_train_steps: the staged sets and indices of a host call, the gathered minibatch, the noise kernel's centred fp64 draws
    // and its staged outputs, the best weights with (loss, step) and what the host knows of them
    DevBuf<float> st0, st1, stt0, stt1, gx0, gx1, gcond, nx1, nout;
    DevBuf<int64_t> idx0, idx1;
    DevBuf<double> nxc, nrot, best_w, best;
    bool best_tracked = false; long long best_steps = 0;      // a call has tracked since the last reset; the steps tracked since then
    bool mirror_stale = false;                   // a many-step call did not reach its read-back: the next one reads the counters first
    // ti_painn_train_set_graphs: the table of gn per-molecule graphs (0: none) -- counts, mask words, pair types (empty: the
    // template's) -- with the host copy of the counts (a call's N), and the flags and counts of the call in flight
    long long gn = 0; std::vector<int32_t> g_nat;
    DevBuf<int32_t> gt_nat, gnat; DevBuf<uint32_t> gt_mask; DevBuf<uint8_t> gt_ptype, gflag;
};

PainnTrainState* state_of(ti_handle* h) { return static_cast<PainnTrainState*>(h->train.get()); }

Plan plan(const PainnTrainState* S, long long B, int halves)
{
    const size_t F = S->d.n_features, A = S->d.n_atoms, E = S->d.n_edges, L = S->d.n_layers;
    const size_t Rn = (size_t)halves * B * A, Re = (size_t)halves * B * E, Rm = std::max(Rn, Re);
    Plan p;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += n; return at; };
    auto rec = [&](size_t rows) { Rec r; r.z1 = take(rows * F); r.y1 = take(rows * F); r.z2 = take(rows * F); r.y2 = take(rows * F); return r; };
    p.xt = take(3 * Rn); p.z = take((size_t)B * 3 * A);
    p.dir = take(3 * Re); p.dist = take(Re); p.enc = take(Re * F); p.s_in0 = take(Rn * S->nE * F); p.emb = rec(Rn);
    p.layers.resize(L);
    p.layers[0].s_in = take(Rn * F); p.layers[0].v_in = take(3 * Rn * F); p.layers[0].e_in = take(Re * F);
    for (size_t l = 0; l < L; ++l) {
        LayerAct& a = p.layers[l];
        a.phi_in = take(2 * Re * F); a.phi = rec(Re); a.P = take(5 * Re * F); a.w = rec(Re); a.Wd = take(5 * Re * F);
        a.s_m = take(Rn * F); a.v_m = take(3 * Rn * F); a.uv = take(3 * Rn * F); a.vv = take(3 * Rn * F); a.up_in = take(2 * Rn * F);
        a.upd = rec(Rn); a.gqa = take(3 * Rn * F); a.s_out = take(Rn * F); a.v_out = take(3 * Rn * F);
        if (l + 1 < L) { p.layers[l + 1].s_in = a.s_out; p.layers[l + 1].v_in = a.v_out; p.layers[l + 1].e_in = take(Re * F); }
    }
    p.ro = rec(Rn); p.ro_out = take(2 * Rn); p.Vv = take(3 * Rn); p.bout = take(3 * Rn);
    p.gb = take(3 * Rn); p.gro = take(2 * Rn); p.gVv = take(3 * Rn);
    for (int k = 0; k < 2; ++k) { p.gs[k] = take(Rn * F); p.gv[k] = take(3 * Rn * F); p.ge[k] = take(Re * F); }
    p.gP = take(5 * Re * F); p.gWd = take(5 * Re * F); p.gin_phi = take(2 * Re * F);
    p.t_gy = take(Rm * F); p.t_gz = take(Rm * F); p.t_gu = take(Rm * F); p.t_gx = take(Rm * F);
    p.gup = take(3 * Rn * F); p.gin_up = take(2 * Rn * F); p.guv = take(3 * Rn * F); p.gvv = take(3 * Rn * F);
    p.tmp1 = take(3 * Rn * F); p.tmp2 = take(3 * Rn * F); p.gin_emb = take(Rn * F);
    p.total = o;
    return p;
}

size_t part64_count(const PainnTrainState* S, long long B)
{
    return (size_t)std::max(std::max(3 * vloss_tiles(B * S->d.n_atoms), vloss_tiles(B)), vloss_tiles((long long)S->nW));
}

// the formula include/ti_hip.h states
unsigned long long workspace_bytes(const PainnTrainState* S, long long B, int halves)
{
    const unsigned long long F = S->d.n_features, A = S->d.n_atoms, E = S->d.n_edges, L = S->d.n_layers, nE = S->nE;
    const unsigned long long Rn = (unsigned long long)halves * B * A, Re = (unsigned long long)halves * B * E, Rm = std::max(Rn, Re);
    const unsigned long long floats = Re * (4 + F * (21 * L + 15)) + Rn * (F * (nE + 23 * L + 38) + 19) + 4 * F * Rm + 3ull * B * A;
    const unsigned long long slices = (unsigned long long)ptrain_slices((long long)std::max(Re, 3 * Rn));
    const unsigned long long col = (unsigned long long)ptrain_slices((long long)Rm) * 5 * F;
    return 4 * floats + 4 * slices * S->max_block + 8 * (col + 6ull * B * A + B + part64_count(S, B));
}

int workspace_check(const PainnTrainState* S, long long B, int halves)
{
    const unsigned long long need = workspace_bytes(S, B, halves), cap = S->max_workspace_bytes ? S->max_workspace_bytes : TI_PAINN_TRAIN_DEFAULT_WORKSPACE;
    if (need > cap)
        return fail(TI_E_UNSUPPORTED, "the call needs a workspace of " + std::to_string(need) + " bytes, above max_workspace_bytes = " + std::to_string(cap));
    return TI_OK;
}

struct Run {        // one call's view of the trainer
    PainnTrainState* S; hipStream_t st; float* ar; PtGraph g;
    int sl_n, sl_e, sl_v;       // slices of a weight gradient over node rows, edge rows, the 3 Rn rows of v

    // out [rows][N] = in [rows][K] W^T (+ bias); W [N][K] canonical
    void lin(const float* in, int K, size_t W, const float* bias, int N, long long rows, float* out) const
    {
        TrGemm q{};
        q.A = in; q.a_si = K; q.a_sk = 1;
        q.B = S->w32.p + W; q.b_sk = 1; q.b_sj = K;
        q.M = rows; q.N = N; q.Kd = K; q.ktile = K;
        q.mode = bias ? TRG_FWD_LIN : TRG_BWD_LIN; q.bias = bias; q.out = out; q.ldo = N;
        HIP_CHECK(launch_train_gemm(q, 1, st));
    }
    // gin [rows][ncol] = gout [rows][N] W[:, :ncol]
    void dgrad(const float* gout, int N, size_t W, int K, int ncol, long long rows, float* gin) const
    {
        TrGemm q{};
        q.A = gout; q.a_si = N; q.a_sk = 1;
        q.B = S->w32.p + W; q.b_sk = K; q.b_sj = 1;
        q.M = rows; q.N = ncol; q.Kd = N; q.ktile = N;
        q.mode = TRG_BWD_LIN; q.out = gin; q.ldo = ncol;
        HIP_CHECK(launch_train_gemm(q, 1, st));
    }
    // slices of dW [N][K] = gout^T in over the rows, into the part buffer of the block that starts at block_off
    void wgrad(const float* gout, int N, const float* in, int K, size_t W, size_t block_off, size_t block_n, long long rows, int slices) const
    {
        TrGemm q{};
        q.A = gout; q.a_si = 1; q.a_sk = N;
        q.B = in; q.b_sk = K; q.b_sj = 1;
        q.M = N; q.N = K; q.Kd = rows; q.ktile = PTRAIN_SLICE;
        q.mode = TRG_WGRAD;
        q.part = S->part.p; q.part_stride = block_n; q.w_off = W - block_off; q.Kin = K;
        HIP_CHECK(launch_train_gemm(q, slices, st));
    }
    void combine(size_t off, size_t n, int slices) const
    {
        HIP_CHECK(launch_train_combine(S->grad.p + off, S->sq.p + off, S->part.p, S->is_bias.p + off, n, n, 0, 0, slices, st));
    }
    void colsum(size_t off, const float* gz, long long rows, int N) const { HIP_CHECK(launch_ptrain_colsum(S->grad.p + off, S->colpart.p, gz, rows, N, st)); }

    void mlp_forward(const MlpOff& m, const float* in, long long rows, const Rec& r, float* out) const
    {
        const float* w = S->w32.p;
        lin(in, m.f_in, m.W0, w + m.b0, m.f_h, rows, ar + r.z1);
        HIP_CHECK(launch_ptrain_ln_fwd(ar + r.y1, ar + r.z1, w + m.g0, w + m.be0, rows, m.f_h, st));
        lin(ar + r.y1, m.f_h, m.W1, w + m.b1, m.f_h, rows, ar + r.z2);
        HIP_CHECK(launch_ptrain_ln_fwd(ar + r.y2, ar + r.z2, w + m.g1, w + m.be1, rows, m.f_h, st));
        lin(ar + r.y2, m.f_h, m.W2, w + m.b2, m.f_out, rows, out);
    }
    // the reverse of mlp_forward from gout [rows][f_out]: every parameter gradient of the block, and gin [rows][ncol] (NULL: none)
    void mlp_backward(const MlpOff& m, const Plan& p, const float* in, long long rows, const Rec& r, const float* gout, float* gin, int ncol,
                      int slices) const
    {
        const float* w = S->w32.p;
        const size_t off = m.W0, n = m.b2 + m.f_out - m.W0;
        float *gy = ar + p.t_gy, *gz = ar + p.t_gz, *gu = ar + p.t_gu, *gx = ar + p.t_gx;
        wgrad(gout, m.f_out, ar + r.y2, m.f_h, m.W2, off, n, rows, slices);
        colsum(m.b2, gout, rows, m.f_out);
        dgrad(gout, m.f_out, m.W2, m.f_h, m.f_h, rows, gy);
        HIP_CHECK(launch_ptrain_ln_bwd(gz, gu, gx, gy, ar + r.z2, w + m.g1, w + m.be1, rows, m.f_h, st));
        colsum(m.g1, gx, rows, m.f_h); colsum(m.be1, gu, rows, m.f_h);
        wgrad(gz, m.f_h, ar + r.y1, m.f_h, m.W1, off, n, rows, slices);
        colsum(m.b1, gz, rows, m.f_h);
        dgrad(gz, m.f_h, m.W1, m.f_h, m.f_h, rows, gy);
        HIP_CHECK(launch_ptrain_ln_bwd(gz, gu, gx, gy, ar + r.z1, w + m.g0, w + m.be0, rows, m.f_h, st));
        colsum(m.g0, gx, rows, m.f_h); colsum(m.be0, gu, rows, m.f_h);
        wgrad(gz, m.f_h, in, m.f_in, m.W0, off, n, rows, slices);
        colsum(m.b0, gz, rows, m.f_h);
        if (gin) dgrad(gz, m.f_h, m.W0, m.f_in, ncol, rows, gin);
        combine(off, n, slices);
    }
};

void ensure_ws(PainnTrainState* S, const Plan& p, long long B, int halves)
{
    const size_t Rn = (size_t)halves * B * S->d.n_atoms, Re = (size_t)halves * B * S->d.n_edges;
    grow(S->arena, p.total);
    grow(S->part, (size_t)ptrain_slices((long long)std::max(Re, 3 * Rn)) * S->max_block);
    grow(S->colpart, (size_t)ptrain_slices((long long)std::max(Re, Rn)) * 5 * S->d.n_features);
    grow(S->raw, (size_t)6 * B * S->d.n_atoms);
    grow(S->loss, (size_t)B);
    grow(S->part64, part64_count(S, B));
    grow(S->t, (size_t)B);
}

// One forward and reverse pass on the device-resident rows (x0, x1 [B][A][3], cond [B][A][ncond]; t, z given or NULL): afterwards
// S->loss holds the loss rows, S->red (their sum, the sum of the squared gradient entries) and S->grad the gradient of the mean loss.
// reverse == false stops behind the loss rows and their sum: S->grad and the sum of squares are left as they were.
void train_forward_backward(ti_handle* h, PainnTrainState* S, const Plan& p, const ti_vloss_desc* d, const float* x0, const float* x1,
                            const float* cond, const float* t_given, const float* z_given, long long B, bool reverse = true,
                            const PtLive* lv = nullptr)
{
    hipStream_t st = h->stream;
    const bool two = d->kind == TI_VLOSS_STANDARD;
    const int halves = two ? 2 : 1, A = S->d.n_atoms, E = S->d.n_edges, F = S->d.n_features, L = S->d.n_layers, m = 3 * A;
    const long long R = (long long)halves * B, Rn = R * A, Re = R * E;
    float* ar = S->arena.p;
    const float* w = S->w32.p;
    Run run{S, st, ar, PtGraph{S->src.p, S->dst.p, A, E, F, R}, (int)ptrain_slices(Rn), (int)ptrain_slices(Re), (int)ptrain_slices(3 * Rn)};
    const PtGraph& g = run.g;

    // ---- states: the velocity loss's interpolate and centre kernels
    const float* td = t_given;
    if (d->t_dist != TI_TDIST_GIVEN) {
        HIP_CHECK(launch_vloss_draw_t(S->t.p, d->t_dist, d->seed, d->traj_offset, d->draw, B, st));
        td = S->t.p;
    }
    const size_t n = (size_t)B * m;
    VlossParams vp{};
    vp.kind = d->kind; vp.gamma = d->gamma; vp.center = d->center; vp.a = d->a;
    vp.B = B; vp.m = m; vp.A = A;
    vp.x0 = x0; vp.x1 = x1; vp.t = td; vp.z_in = z_given;
    vp.seed = d->seed; vp.traj0 = d->traj_offset; vp.draw = d->draw;
    vp.z = two ? ar + p.z : nullptr; vp.raw = S->raw.p; vp.colsum = S->red.p + RED_COLSUM;
    vp.xt = ar + p.xt; vp.half = (long long)n;
    HIP_CHECK(lv ? launch_ptg_interp(vp, *lv, st) : launch_vloss_interp(vp, st));
    if (d->center == TI_CENTER_BATCH)
        for (int hf = 0; hf < halves; ++hf)
            HIP_CHECK(launch_vloss_colsum(S->red.p + RED_COLSUM + hf * 3, S->part64.p, S->raw.p + (size_t)hf * n, B * A, 3, st));
    if (d->center != TI_CENTER_NONE) HIP_CHECK(lv ? launch_ptg_center(vp, *lv, st) : launch_vloss_center(vp, st));
    if (lv) HIP_CHECK(launch_ptg_pad(ar + p.xt, (long long)n, halves, A, *lv, st));

    // ---- forward
    HIP_CHECK(launch_ptrain_geom(ar + p.dir, ar + p.dist, ar + p.xt, g, st));
    HIP_CHECK(launch_ptrain_enc(ar + p.enc, ar + p.dist, S->d.length_scale, g, st));
    PtEmbedIn ei{w + S->atom_emb, cond, td, S->atom_ids.p, S->ncond, S->nE, B, S->d.temp_length, S->d.time_length, S->d.temp_mean, S->d.temp_range};
    HIP_CHECK(lv ? launch_ptg_embed_in(ar + p.s_in0, ei, g, *lv, st) : launch_ptrain_embed_in(ar + p.s_in0, ei, g, st));
    HIP_CHECK(lv ? launch_ptg_edge_emb(ar + p.layers[0].e_in, w + S->edge_emb, g, *lv, st)
                 : launch_ptrain_edge_emb(ar + p.layers[0].e_in, w + S->edge_emb, S->etype.p, g, st));
    HIP_CHECK(hipMemsetAsync(ar + p.layers[0].v_in, 0, (size_t)3 * Rn * F * sizeof(float), st));
    run.mlp_forward(S->embed, ar + p.s_in0, Rn, p.emb, ar + p.layers[0].s_in);
    for (int l = 0; l < L; ++l) {
        const LayerAct& a = p.layers[l];
        HIP_CHECK(launch_ptrain_phi_in(ar + a.phi_in, ar + a.s_in, ar + a.e_in, g, st));
        run.mlp_forward(S->phi[l], ar + a.phi_in, Re, a.phi, ar + a.P);
        run.mlp_forward(S->filt[l], ar + p.enc, Re, a.w, ar + a.Wd);
        HIP_CHECK(lv ? launch_ptg_msg_fwd(ar + a.s_m, ar + a.v_m, ar + a.s_in, ar + a.v_in, ar + a.P, ar + a.Wd, ar + p.dir, g, *lv, st)
                     : launch_ptrain_msg_fwd(ar + a.s_m, ar + a.v_m, ar + a.s_in, ar + a.v_in, ar + a.P, ar + a.Wd, ar + p.dir, g, st));
        if (l + 1 < L) HIP_CHECK(launch_ptrain_e_fwd(ar + p.layers[l + 1].e_in, ar + a.e_in, ar + a.P, ar + a.Wd, g, st));
        run.lin(ar + a.v_m, F, S->U[l], nullptr, F, 3 * Rn, ar + a.uv);
        run.lin(ar + a.v_m, F, S->V[l], nullptr, F, 3 * Rn, ar + a.vv);
        HIP_CHECK(launch_ptrain_upd_in(ar + a.up_in, ar + a.vv, ar + a.s_m, g, st));
        run.mlp_forward(S->upd[l], ar + a.up_in, Rn, a.upd, ar + a.gqa);
        HIP_CHECK(launch_ptrain_upd_apply(ar + a.s_out, ar + a.v_out, ar + a.s_m, ar + a.v_m, ar + a.uv, ar + a.up_in, ar + a.gqa, g, st));
    }
    const float *s_fin = ar + p.layers[L - 1].s_out, *v_fin = ar + p.layers[L - 1].v_out;
    run.mlp_forward(S->readout, s_fin, Rn, p.ro, ar + p.ro_out);
    run.lin(v_fin, F, S->Vr, nullptr, 1, 3 * Rn, ar + p.Vv);
    HIP_CHECK(launch_ptrain_readout(ar + p.bout, ar + p.Vv, ar + p.ro_out, Rn, st));

    // ---- the loss rows by the velocity loss's own kernel, their sum by its fixed tree
    vp.b = ar + p.bout; vp.loss = S->loss.p;
    HIP_CHECK(lv ? launch_ptg_reduce(vp, *lv, st) : launch_vloss_reduce(vp, st));
    HIP_CHECK(launch_vloss_colsum(S->red.p + RED_LOSS, S->part64.p, S->loss.p, B, 1, st));
    if (!reverse) return;

    // ---- reverse
    HIP_CHECK(lv ? launch_ptg_gout(ar + p.gb, vp, *lv, st) : launch_ptrain_gout(ar + p.gb, vp, st));
    int cur = 0;
    HIP_CHECK(launch_ptrain_readout_bwd(ar + p.gro, ar + p.gVv, ar + p.gv[cur], ar + p.gb, ar + p.Vv, ar + p.ro_out, w + S->Vr, g, st));
    run.wgrad(ar + p.gVv, 1, v_fin, F, S->Vr, S->Vr, (size_t)F, 3 * Rn, run.sl_v);
    run.combine(S->Vr, (size_t)F, run.sl_v);
    run.mlp_backward(S->readout, p, s_fin, Rn, p.ro, ar + p.gro, ar + p.gs[cur], F, run.sl_n);
    const float* ge = nullptr;          // the last layer's e is not read: its de chunk gets no gradient
    int ecur = 0;
    for (int l = L - 1; l >= 0; --l) {
        const LayerAct& a = p.layers[l];
        // update
        HIP_CHECK(launch_ptrain_upd_bwd_a(ar + p.gup, ar + p.guv, ar + p.gs[cur], ar + p.gv[cur], ar + a.uv, ar + a.up_in, ar + a.gqa, g, st));
        run.mlp_backward(S->upd[l], p, ar + a.up_in, Rn, a.upd, ar + p.gup, ar + p.gin_up, 2 * F, run.sl_n);
        HIP_CHECK(launch_ptrain_upd_bwd_b(ar + p.gvv, ar + p.gs[1 - cur], ar + p.gs[cur], ar + p.gin_up, ar + a.vv, ar + a.up_in, ar + a.gqa, g, st));
        const size_t uv_n = (size_t)2 * F * F;
        run.wgrad(ar + p.guv, F, ar + a.v_m, F, S->U[l], S->U[l], uv_n, 3 * Rn, run.sl_v);
        run.wgrad(ar + p.gvv, F, ar + a.v_m, F, S->V[l], S->U[l], uv_n, 3 * Rn, run.sl_v);
        run.combine(S->U[l], uv_n, run.sl_v);
        run.dgrad(ar + p.guv, F, S->U[l], F, F, 3 * Rn, ar + p.tmp1);
        run.dgrad(ar + p.gvv, F, S->V[l], F, F, 3 * Rn, ar + p.tmp2);
        HIP_CHECK(launch_ptrain_add3(ar + p.gv[1 - cur], ar + p.gv[cur], ar + p.tmp1, ar + p.tmp2, 3 * Rn * F, st));
        cur = 1 - cur;
        // message
        HIP_CHECK(lv ? launch_ptg_msg_bwd_edge(ar + p.gP, ar + p.gWd, ar + p.gs[cur], ar + p.gv[cur], ge, ar + a.v_in, ar + a.P, ar + a.Wd, ar + p.dir, g, *lv, st)
                     : launch_ptrain_msg_bwd_edge(ar + p.gP, ar + p.gWd, ar + p.gs[cur], ar + p.gv[cur], ge, ar + a.v_in, ar + a.P, ar + a.Wd, ar + p.dir, g, st));
        run.mlp_backward(S->phi[l], p, ar + a.phi_in, Re, a.phi, ar + p.gP, ar + p.gin_phi, 2 * F, run.sl_e);
        run.mlp_backward(S->filt[l], p, ar + p.enc, Re, a.w, ar + p.gWd, nullptr, 0, run.sl_e);
        HIP_CHECK(lv ? launch_ptg_msg_bwd_node(ar + p.gs[1 - cur], ar + p.gv[1 - cur], ar + p.gs[cur], ar + p.gv[cur], ar + p.gin_phi, ar + a.P, ar + a.Wd,
                                               ar + p.dir, g, *lv, st)
                     : launch_ptrain_msg_bwd_node(ar + p.gs[1 - cur], ar + p.gv[1 - cur], ar + p.gs[cur], ar + p.gv[cur], ar + p.gin_phi, ar + a.P, ar + a.Wd,
                                                  ar + p.dir, g, st));
        HIP_CHECK(launch_ptrain_e_bwd(ar + p.ge[ecur], ge, ar + p.gin_phi, g, st));
        ge = ar + p.ge[ecur]; ecur = 1 - ecur;
        cur = 1 - cur;
    }
    HIP_CHECK(lv ? launch_ptg_table(S->grad.p + S->edge_emb, ge, F, g, *lv, st)
                 : launch_ptrain_table(S->grad.p + S->edge_emb, ge, F, S->etype.p, E, 4, R, F, st));
    run.mlp_backward(S->embed, p, ar + p.s_in0, Rn, p.emb, ar + p.gs[cur], ar + p.gin_emb, F, run.sl_n);
    HIP_CHECK(launch_ptrain_table(S->grad.p + S->atom_emb, ar + p.gin_emb, F, S->atom_ids.p, A, S->d.n_types, R, F, st));
    HIP_CHECK(launch_train_combine(S->grad.p, S->sq.p, nullptr, S->is_bias.p, 0, S->nW, 0, 0, 0, st));
    HIP_CHECK(launch_vloss_colsum(S->red.p + RED_SUMSQ, S->part64.p, S->sq.p, (long long)S->nW, 1, st));
}

// the checks ti_painn_train_grad and ti_painn_train_step share, in the order include/ti_hip.h lists them
int call_check(ti_handle* h, const ti_vloss_desc* d, const float* x0, const float* x1, const float* cond, const float* t, const float* z, int64_t B,
               int mem)
{
    if (int rc = vloss_check(d, t, z, B, mem)) return rc;
    const bool ours = h && h->kind == 3;
    if (ours) if (int rc = workspace_check(state_of(h), B, d->kind == TI_VLOSS_STANDARD ? 2 : 1)) return rc;
    if (!x0 || !x1 || (ours && state_of(h)->ncond > 0 && !cond)) return fail(TI_E_ARG, "NULL buffer");
    if (!ours) return fail(TI_E_ARG, "not a painn trainer handle");
    if (state_of(h)->gn && state_of(h)->gn != B)
        return fail(TI_E_ARG, "the table of ti_painn_train_set_graphs has " + std::to_string(state_of(h)->gn) + " rows, the call B = " + std::to_string(B));
    return TI_OK;
}

// With a table in force: the flags and counts of a call over B molecules that reads the table rows idx (idx_dev where the kernel
// reads them, idx_host for N; both NULL: rows 0..B-1), enqueued on the stream.  gflag and gnat have been grown by the caller.
PtLive expand_graphs(ti_handle* h, PainnTrainState* S, const long long* idx_dev, const int64_t* idx_host, long long B)
{
    const PtTable t{S->gt_nat.p, S->gt_mask.p, S->gt_ptype.p, idx_dev, S->gn};
    const PtGraph g{S->src.p, S->dst.p, S->d.n_atoms, S->d.n_edges, S->d.n_features, 0};
    HIP_CHECK(launch_ptg_expand(S->gflag.p, S->gnat.p, t, S->etype.p, g, B, h->stream));
    long long N = 0;
    for (long long b = 0; b < B; ++b) N += S->g_nat[(size_t)(idx_host ? idx_host[b] : b)];
    return PtLive{S->gflag.p, S->gnat.p, B, (double)N};
}

void grow_graph_flags(PainnTrainState* S, long long B)
{
    grow(S->gflag, (size_t)B * S->d.n_edges);
    grow(S->gnat, (size_t)B);
}

// stages the inputs of a host call and runs the two passes -> the divisor of the mean: B A, or N with a table in force
double run_passes(ti_handle* h, PainnTrainState* S, const ti_vloss_desc* d, const float* x0, const float* x1, const float* cond, const float* t,
                  const float* z, int64_t B, int mem)
{
    Staged sg(h, mem);
    const int halves = d->kind == TI_VLOSS_STANDARD ? 2 : 1;
    const size_t n = (size_t)B * 3 * S->d.n_atoms;
    const Plan p = plan(S, B, halves);
    ensure_ws(S, p, B, halves);
    const float *x0d = sg.in(x0, S->sx0, n), *x1d = sg.in(x1, S->sx1, n);
    const float* cd = sg.in(cond, S->sc, (size_t)B * S->d.n_atoms * S->ncond);
    const float *td = sg.in(t, S->tin, (size_t)B), *zd = sg.in(z, S->zin, n);
    if (!S->gn) { train_forward_backward(h, S, p, d, x0d, x1d, cd, td, zd, B); return (double)(B * S->d.n_atoms); }
    grow_graph_flags(S, B);
    const PtLive lv = expand_graphs(h, S, nullptr, nullptr, B);
    train_forward_backward(h, S, p, d, x0d, x1d, cd, td, zd, B, true, &lv);
    return lv.N;
}

}  // namespace

extern "C" {

ti_handle* ti_painn_trainer_create(const ti_painn_desc* d, const double* weights, size_t n_weights, const int32_t* edge_src,
                                   const int32_t* edge_dst, const int32_t* edge_type, const int32_t* atom_ids,
                                   const ti_painn_train_desc* td, int device)
{
    ti_handle* out = nullptr;
    const int rc = guarded([&]() -> int {
        if (!d || !weights || !atom_ids) return fail(TI_E_ARG, "NULL argument");
        const int F = d->n_features, L = d->n_layers, A = d->n_atoms, E = d->n_edges;
        if (F != 32 && F != 64 && F != 128 && F != 256) return fail(TI_E_UNSUPPORTED, "n_features must be 32, 64, 128 or 256");
        if (L < 1) return fail(TI_E_ARG, "n_layers must be >= 1");
        if (A < 1 || A > 32) return fail(TI_E_UNSUPPORTED, "n_atoms must be in 1..32 (the reference caps it at n_types = 25)");
        if (E < 0 || (E > 0 && (!edge_src || !edge_dst || !edge_type))) return fail(TI_E_ARG, "edge arrays missing");
        if (d->variant < 0 || d->variant > 2) return fail(TI_E_ARG, "unknown variant");
        if (d->n_types < 1) return fail(TI_E_ARG, "n_types must be >= 1");
        if (d->precision != TI_PREC_F32 && d->precision != TI_PREC_F16X2 && d->precision != TI_PREC_F16) return fail(TI_E_ARG, "unknown precision");
        for (int k = 0; k < E; ++k)
            if (edge_src[k] < 0 || edge_src[k] >= A || edge_dst[k] < 0 || edge_dst[k] >= A || edge_type[k] < 0 || edge_type[k] > 3)
                return fail(TI_E_ARG, "edge index / type out of range");
        for (int a = 0; a < A; ++a) if (atom_ids[a] < 0 || atom_ids[a] >= d->n_types) return fail(TI_E_ARG, "atom id out of range");
        auto S = std::make_shared<PainnTrainState>();
        S->d = *d;
        S->nE = d->variant == TI_VARIANT_AMBIENT ? 4 : d->variant == TI_VARIANT_LATENT_MULTI ? 3 : 2;
        S->ncond = d->variant == TI_VARIANT_AMBIENT ? 2 : d->variant == TI_VARIANT_LATENT_MULTI ? 1 : 0;
        size_t o = 0;
        S->edge_emb = o; o += 4 * (size_t)F; S->atom_emb = o; o += (size_t)d->n_types * F;
        o = take_mlp(S->embed, o, S->nE * F, F, F);
        S->phi.resize(L); S->filt.resize(L); S->upd.resize(L); S->U.resize(L); S->V.resize(L);
        for (int l = 0; l < L; ++l) {
            o = take_mlp(S->phi[l], o, 2 * F, F, 5 * F); o = take_mlp(S->filt[l], o, F, F, 5 * F);
            S->U[l] = o; o += (size_t)F * F; S->V[l] = o; o += (size_t)F * F;
            o = take_mlp(S->upd[l], o, 2 * F, F, 3 * F);
        }
        o = take_mlp(S->readout, o, F, F, 2);
        S->Vr = o; o += F;
        if (o != n_weights) return fail(TI_E_ARG, "weight count mismatch: expected " + std::to_string(o) + ", got " + std::to_string(n_weights));
        if (d->precision != TI_PREC_F32) return fail(TI_E_UNSUPPORTED, "the trainer takes TI_PREC_F32 only");
        if (E == 0) return fail(TI_E_UNSUPPORTED, "the trainer needs an edge template: n_edges == 0");
        if (!td) return fail(TI_E_ARG, "train desc is NULL");
        const AdamDesc ad{td->lr, td->beta1, td->beta2, td->eps, td->weight_decay, td->max_grad_norm};
        if (int rc2 = adam_desc_check(ad)) return rc2;
        S->max_workspace_bytes = td->max_workspace_bytes;
        S->max_block = (size_t)8 * F * F + (size_t)11 * F;          // phi's MLP, the largest parameter block
        std::unique_ptr<ti_handle> h(new_handle(3, device));
        h->d = *d;
        std::vector<unsigned char> mask(o, 1);
        auto weights_of = [&](const MlpOff& m) {
            std::fill(mask.begin() + m.W0, mask.begin() + m.b0, (unsigned char)0);
            std::fill(mask.begin() + m.W1, mask.begin() + m.b1, (unsigned char)0);
            std::fill(mask.begin() + m.W2, mask.begin() + m.b2, (unsigned char)0);
        };
        weights_of(S->embed); weights_of(S->readout);
        for (int l = 0; l < L; ++l) {
            weights_of(S->phi[l]); weights_of(S->filt[l]); weights_of(S->upd[l]);
            std::fill(mask.begin() + S->U[l], mask.begin() + S->U[l] + (size_t)2 * F * F, (unsigned char)0);
        }
        std::fill(mask.begin() + S->Vr, mask.begin() + S->Vr + F, (unsigned char)0);
        S->setup(ad, weights, mask, 8, 1, h->stream);
        S->src.upload(std::vector<int32_t>(edge_src, edge_src + E)); S->dst.upload(std::vector<int32_t>(edge_dst, edge_dst + E));
        S->etype.upload(std::vector<int32_t>(edge_type, edge_type + E)); S->atom_ids.upload(std::vector<int32_t>(atom_ids, atom_ids + A));
        h->train = S;
        out = h.release();
        return TI_OK;
    });
    return rc == TI_OK ? out : nullptr;
}

int ti_painn_train_grad(ti_handle* h, const ti_vloss_desc* d, const float* x0, const float* x1, const float* cond, const float* t,
                        const float* z, int64_t B, double* out_loss, double* out_mean, double* out_grad, double* out_gnorm, int mem)
{
    if (int rc = call_check(h, d, x0, x1, cond, t, z, B, mem)) return rc;
    return guarded([&]() -> int {
        set_device(h);
        PainnTrainState* S = state_of(h);
        const double divisor = run_passes(h, S, d, x0, x1, cond, t, z, B, mem);
        return S->grad_readback(out_loss, out_mean, out_grad, out_gnorm, B, divisor, mem, S->loss.p, h->stream);
    });
}

int ti_painn_train_apply(ti_handle* h, const double* grad, int32_t* out_skipped)
{
    if (!grad) return fail(TI_E_ARG, "NULL buffer");
    if (!h || h->kind != 3) return fail(TI_E_ARG, "not a painn trainer handle");
    return guarded([&]() -> int { set_device(h); return state_of(h)->apply(grad, out_skipped, 0, h->stream); });
}

int ti_painn_train_step(ti_handle* h, const ti_vloss_desc* d, const float* x0, const float* x1, const float* cond, const float* t,
                        const float* z, int64_t B, double* out_mean, int32_t* out_skipped, int mem)
{
    if (int rc = call_check(h, d, x0, x1, cond, t, z, B, mem)) return rc;
    return guarded([&]() -> int {
        set_device(h);
        PainnTrainState* S = state_of(h);
        hipStream_t st = h->stream;
        S->read_counters(st);
        S->upload_bias(1, st);
        const double divisor = run_passes(h, S, d, x0, x1, cond, t, z, B, mem);
        const TrAdam a = S->adam_params(true, divisor, S->log.p);
        HIP_CHECK(launch_train_adam(a, st));
        HIP_CHECK(launch_train_finish(a, st));
        double mean = 0.0;
        HIP_CHECK(hipMemcpyAsync(&mean, S->log.p, sizeof(double), hipMemcpyDeviceToHost, st));
        const long long before = S->n_skipped;
        S->read_counters(st);
        if (out_mean) *out_mean = mean;
        if (out_skipped) *out_skipped = (int32_t)(S->n_skipped - before);
        return TI_OK;
    });
}

int ti_painn_train_get_state(ti_handle* h, double* w, double* m, double* v, int64_t* n_applied, int64_t* n_skipped)
{
    if (!h || h->kind != 3) return fail(TI_E_ARG, "not a painn trainer handle");
    return guarded([&]() -> int { set_device(h); return state_of(h)->get_state(w, m, v, n_applied, n_skipped, h->stream); });
}

int ti_painn_train_set_state(ti_handle* h, const double* w, const double* m, const double* v, int64_t n_applied)
{
    if (n_applied < 0) return fail(TI_E_ARG, "n_applied < 0");
    if (!h || h->kind != 3) return fail(TI_E_ARG, "not a painn trainer handle");
    return guarded([&]() -> int { set_device(h); return state_of(h)->set_state(w, m, v, n_applied, h->stream); });
}

int ti_painn_train_set_lr(ti_handle* h, double lr)
{
    if (int rc = lr_check(lr)) return rc;
    if (!h || h->kind != 3) return fail(TI_E_ARG, "not a painn trainer handle");
    state_of(h)->td.lr = lr;
    return TI_OK;
}

int64_t ti_painn_train_workspace_bytes(ti_handle* h, int64_t B, int32_t kind)
{
    if (B < 1 || (kind != TI_VLOSS_STANDARD && kind != TI_VLOSS_ONE_SIDED)) return fail(TI_E_ARG, "B < 1 or an unknown loss kind");
    if (!h || h->kind != 3) return fail(TI_E_ARG, "not a painn trainer handle");
    return (int64_t)workspace_bytes(state_of(h), B, kind == TI_VLOSS_STANDARD ? 2 : 1);
}

int ti_painn_train_steps(ti_handle* h, const ti_vloss_desc* d, const ti_painn_steps_desc* sd, const float* x0, int64_t n0, const float* temp0,
                         const float* x1, int64_t n1, const float* temp1, const int64_t* idx0, const int64_t* idx1, int64_t B,
                         double* out_loss, int64_t* out_skipped, int mem)
{
    if (int rc = vloss_check(d, nullptr, nullptr, B, mem)) return rc;
    if (!sd) return fail(TI_E_ARG, "steps desc is NULL");
    if (sd->n_steps < 1 || sd->n_steps > INT32_MAX) return fail(TI_E_ARG, "n_steps must be in 1..2^31 - 1");
    if (sd->update != 0 && sd->update != 1) return fail(TI_E_ARG, "unknown update " + std::to_string(sd->update));
    if (sd->noise < TI_NOISE_GIVEN || sd->noise > TI_NOISE_ALIGNED) return fail(TI_E_ARG, "unknown noise " + std::to_string(sd->noise));
    if (sd->track_best != 0 && sd->track_best != 1) return fail(TI_E_ARG, "unknown track_best " + std::to_string(sd->track_best));
    const bool given = sd->noise == TI_NOISE_GIVEN;
    if (!given && d->kind != TI_VLOSS_ONE_SIDED) return fail(TI_E_ARG, "drawn noise is the one-sided loss's x0: the loss kind must be ONE_SIDED");
    if (!given && x0) return fail(TI_E_ARG, "x0 is drawn by this noise: x0 must be NULL");
    if (sd->track_best && !sd->update) return fail(TI_E_ARG, "track_best needs update == 1");
    const bool ours = h && h->kind == 3;
    if (ours) if (int rc = workspace_check(state_of(h), B, d->kind == TI_VLOSS_STANDARD ? 2 : 1)) return rc;
    const int64_t n_steps = sd->n_steps;
    if ((idx0 == nullptr) != (idx1 == nullptr)) return fail(TI_E_ARG, "idx0 and idx1 must both be given or both be NULL");
    if (!idx0 && n_steps != 1) return fail(TI_E_ARG, "without indices n_steps must be 1");
    if (n1 < 1 || (given && n0 < 1) || (!idx0 && (n1 < B || (given && n0 < B)))) return fail(TI_E_ARG, "n0 / n1 do not cover the rows of a step");
    if ((long long)d->draw + (n_steps - 1) > INT32_MAX) return fail(TI_E_ARG, "draw + n_steps overflows the draw index");
    if (!x1 || (given && !x0)) return fail(TI_E_ARG, "NULL buffer");
    if (ours) {
        const int nc = state_of(h)->ncond;
        if ((nc >= 1 && !temp1) || (nc == 2 && !temp0)) return fail(TI_E_ARG, "NULL temperature buffer");
        if (nc == 0 && (temp0 || temp1)) return fail(TI_E_ARG, "the single-T variant takes no temperatures: temp0 and temp1 must be NULL");
    }
    const size_t n_idx = idx0 ? (size_t)n_steps * (size_t)B : 0;
    if (idx0 && mem == TI_MEM_HOST) if (int rc = train_idx_check(idx0, idx1, n_idx, n0, n1, given, mem)) return rc;
    if (!ours) return fail(TI_E_ARG, "not a painn trainer handle");
    if (!given && state_of(h)->ncond == 2) return fail(TI_E_UNSUPPORTED, "drawn noise on the ambient variant: its set 0 is data");
    if (sd->noise == TI_NOISE_ALIGNED && h->d.n_atoms < 3) return fail(TI_E_UNSUPPORTED, "TI_NOISE_ALIGNED needs n_atoms >= 3: the rotation is not unique");
    if (state_of(h)->gn && !given) return fail(TI_E_UNSUPPORTED, "a table of ti_painn_train_set_graphs is in force: drawn base samples on per-molecule graphs are not built");
    if (state_of(h)->gn && state_of(h)->gn != n0)
        return fail(TI_E_ARG, "the table of ti_painn_train_set_graphs has " + std::to_string(state_of(h)->gn) + " rows, set 0 n0 = " + std::to_string(n0));
    return guarded([&]() -> int {
        set_device(h);
        PainnTrainState* S = state_of(h);
        hipStream_t st = h->stream;
        Staged sg(h, mem);
        const bool update = sd->update == 1;
        const int A = S->d.n_atoms, halves = d->kind == TI_VLOSS_STANDARD ? 2 : 1;
        const size_t m = (size_t)3 * A;
        if (idx0 && !sg.host) if (int rc = train_idx_check(idx0, idx1, n_idx, n0, n1, given, mem)) return rc;      // nothing has been enqueued yet
        const Plan p = plan(S, B, halves);
        ensure_ws(S, p, B, halves);
        grow(S->log, (size_t)n_steps);
        // a table in force: the rows a step reads are idx0's, which the host needs for the step's N (device indices are read back here,
        // before anything is enqueued)
        std::vector<int64_t> gidx;
        const int64_t* gidx_h = nullptr;
        if (S->gn) {
            grow_graph_flags(S, B);
            if (idx0 && sg.host) gidx_h = idx0;
            else if (idx0) {
                gidx.resize(n_idx);
                HIP_CHECK(hipMemcpy(gidx.data(), idx0, n_idx * sizeof(int64_t), hipMemcpyDeviceToHost));
                gidx_h = gidx.data();
            }
        }
        grow(S->gx0, (size_t)B * m); grow(S->gx1, (size_t)B * m); grow(S->gcond, (size_t)B * A * std::max(S->ncond, 1));
        if (!given) grow(S->nxc, (size_t)B * m);
        if (sd->track_best && !S->best_w.p) {
            S->best_w.alloc(S->nW); S->best.alloc(2);
            static const double init[2] = {HUGE_VAL, -1.0};
            HIP_CHECK(hipMemcpyAsync(S->best.p, init, sizeof(init), hipMemcpyHostToDevice, st));
        }
        const float *x0d = given ? sg.in(x0, S->st0, (size_t)n0 * m) : nullptr, *x1d = sg.in(x1, S->st1, (size_t)n1 * m);
        const float *t0d = S->ncond == 2 ? sg.in(temp0, S->stt0, (size_t)n0) : nullptr;
        const float *t1d = S->ncond >= 1 ? sg.in(temp1, S->stt1, (size_t)n1) : nullptr;
        const long long *i0d = idx_ll(sg.in(idx0, S->idx0, n_idx)), *i1d = idx_ll(sg.in(idx1, S->idx1, n_idx));
        // the bias table and the log are indexed from the host mirror of the counters, which every stepping call brings up to date at
        // its end; only a call that failed half-way leaves it behind, and then the counters are read first
        if (S->mirror_stale) S->read_counters(st);
        S->mirror_stale = true;
        if (update) S->upload_bias(n_steps, st);
        const double divisor = (double)(B * A);
        const TrAdam a = S->adam_params(true, divisor, S->log.p);
        ti_vloss_desc dk = *d;
        for (int64_t k = 0; k < n_steps; ++k) {
            dk.draw = d->draw + (int32_t)k;
            PtGather g{};
            g.gx0 = S->gx0.p; g.gx1 = S->gx1.p; g.cond = S->gcond.p;
            g.x0 = x0d; g.x1 = x1d; g.temp0 = t0d; g.temp1 = t1d;
            g.idx0 = given && i0d ? i0d + k * B : nullptr; g.idx1 = i1d ? i1d + k * B : nullptr;
            g.n0 = given ? n0 : B; g.n1 = n1; g.B = B; g.A = A; g.ncond = S->ncond;
            HIP_CHECK(launch_ptsteps_gather(g, st));
            if (!given) {
                PtNoise q{dk.seed, dk.traj_offset, dk.draw, S->gx1.p, B, A, sd->noise == TI_NOISE_ALIGNED ? 1 : 0, S->nxc.p, S->gx0.p, nullptr};
                HIP_CHECK(launch_ptnoise(q, st));
            }
            double div_k = divisor;
            TrAdam ak = a;
            if (S->gn) {
                const PtLive lv = expand_graphs(h, S, g.idx0, gidx_h ? gidx_h + k * B : nullptr, B);
                div_k = ak.B = lv.N;
                train_forward_backward(h, S, p, &dk, S->gx0.p, S->gx1.p, S->ncond ? S->gcond.p : nullptr, nullptr, nullptr, B, update, &lv);
            } else train_forward_backward(h, S, p, &dk, S->gx0.p, S->gx1.p, S->ncond ? S->gcond.p : nullptr, nullptr, nullptr, B, update);
            if (!update) { HIP_CHECK(launch_ptsteps_log(S->log.p + k, S->red.p + RED_LOSS, div_k, st)); continue; }
            if (sd->track_best) {
                const PtBest q{S->best_w.p, S->w.p, S->nW, S->best.p, S->red.p + RED_LOSS, S->red.p + RED_SUMSQ, div_k, (double)(S->best_steps + k)};
                HIP_CHECK(launch_ptsteps_best_keep(q, st));
                HIP_CHECK(launch_ptsteps_best_commit(q, st));
            }
            HIP_CHECK(launch_train_adam(ak, st));
            HIP_CHECK(launch_train_finish(ak, st));
        }
        S->steps_readback(out_loss, out_skipped, n_steps, st);      // the one synchronisation of the call
        S->mirror_stale = false;
        if (sd->track_best) { S->best_tracked = true; S->best_steps += n_steps; }
        return TI_OK;
    });
}

int ti_painn_train_best(ti_handle* h, double* w, double* loss, int64_t* step, int reset)
{
    if (!h || h->kind != 3) return fail(TI_E_ARG, "not a painn trainer handle");
    PainnTrainState* S = state_of(h);
    if (!S->best_tracked) return fail(TI_E_ARG, "no step has been tracked since the last reset");
    return guarded([&]() -> int {
        set_device(h);
        double meta[2] = {0.0, 0.0};
        HIP_CHECK(hipMemcpyAsync(meta, S->best.p, sizeof(meta), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (w && meta[1] >= 0.0) {
            HIP_CHECK(hipMemcpyAsync(w, S->best_w.p, S->nW * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        if (loss) *loss = meta[0];
        if (step) *step = (int64_t)meta[1];
        if (reset) {
            const double init[2] = {HUGE_VAL, -1.0};
            HIP_CHECK(hipMemcpyAsync(S->best.p, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
            S->best_tracked = false; S->best_steps = 0;
        }
        return TI_OK;
    });
}

int ti_painn_train_noise(ti_handle* h, uint64_t seed, int64_t traj_offset, int32_t draw, const float* x1, int64_t B, int32_t noise,
                         float* out_x0, double* out_rot, int mem)
{
    if (noise != TI_NOISE_DRAWN && noise != TI_NOISE_ALIGNED) return fail(TI_E_ARG, "noise must be TI_NOISE_DRAWN or TI_NOISE_ALIGNED");
    if (B < 1) return fail(TI_E_ARG, "B < 1");
    if (draw < 0) return fail(TI_E_ARG, "draw < 0");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (!out_x0) return fail(TI_E_ARG, "NULL buffer");
    const bool aligned = noise == TI_NOISE_ALIGNED;
    if (aligned && !x1) return fail(TI_E_ARG, "TI_NOISE_ALIGNED needs x1");
    if (!h || h->kind != 3) return fail(TI_E_ARG, "not a painn trainer handle");
    if (aligned && h->d.n_atoms < 3) return fail(TI_E_UNSUPPORTED, "TI_NOISE_ALIGNED needs n_atoms >= 3: the rotation is not unique");
    return guarded([&]() -> int {
        set_device(h);
        PainnTrainState* S = state_of(h);
        hipStream_t st = h->stream;
        const bool host = mem == TI_MEM_HOST;
        const size_t n = (size_t)B * 3 * S->d.n_atoms;
        grow(S->nxc, n);
        const float* x1d = aligned ? Staged(h, mem).in(x1, S->nx1, n) : nullptr;
        float* od = out_x0; double* rd = aligned ? out_rot : nullptr;
        if (host) {
            grow(S->nout, n); od = S->nout.p;
            if (rd) { grow(S->nrot, (size_t)B * 9); rd = S->nrot.p; }
        }
        const PtNoise q{seed, traj_offset, draw, x1d, B, S->d.n_atoms, aligned ? 1 : 0, S->nxc.p, od, rd};
        HIP_CHECK(launch_ptnoise(q, st));
        if (host) {
            HIP_CHECK(hipMemcpyAsync(out_x0, od, n * sizeof(float), hipMemcpyDeviceToHost, st));
            if (rd) HIP_CHECK(hipMemcpyAsync(out_rot, rd, (size_t)B * 9 * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        return TI_OK;
    });
}

int ti_painn_train_set_graphs(ti_handle* h, const int32_t* n_atoms, const uint32_t* mask, const uint8_t* pair_type, int64_t n, int mem)
{
    if (!h || h->kind != 3) return fail(TI_E_ARG, "not a painn trainer handle");
    const bool any = n_atoms || mask || pair_type;
    if (any && n < 1) return fail(TI_E_ARG, "n < 1");
    PainnTrainState* S = state_of(h);
    const int A = S->d.n_atoms;
    auto counts_check = [&](const int32_t* na) {
        for (int64_t b = 0; na && b < n; ++b)
            if (na[b] < 1 || na[b] > A) return fail(TI_E_ARG, "n_atoms[" + std::to_string(b) + "] = " + std::to_string(na[b]) + " is outside 1.." + std::to_string(A));
        return (int)TI_OK;
    };
    auto types_check = [&](const uint8_t* pt) {
        const size_t per = (size_t)A * A;
        for (size_t i = 0; pt && i < (size_t)n * per; ++i) if (pt[i] > 3) return fail(TI_E_ARG, "pair_type above 3 (molecule " + std::to_string(i / per) + ")");
        return (int)TI_OK;
    };
    if (any && mem != TI_MEM_DEVICE) {      // the stated order puts these ahead of the mem check: what is not TI_MEM_DEVICE is read as host arrays
        if (int rc = counts_check(n_atoms)) return rc;
        if (int rc = types_check(pair_type)) return rc;
    }
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    return guarded([&]() -> int {
        set_device(h);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (!any) {
            S->gn = 0; S->g_nat.clear();
            S->gt_nat.release(); S->gt_mask.release(); S->gt_ptype.release();
            return TI_OK;
        }
        auto fetch = [&](void* dst, const void* src, size_t bytes) {
            if (mem == TI_MEM_DEVICE) HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            else std::memcpy(dst, src, bytes);
        };
        std::vector<int32_t> na((size_t)n, A);
        if (n_atoms) fetch(na.data(), n_atoms, na.size() * sizeof(int32_t));
        std::vector<uint8_t> pt;
        if (pair_type) { pt.resize((size_t)n * A * A); fetch(pt.data(), pair_type, pt.size()); }
        if (mem == TI_MEM_DEVICE) {
            if (int rc = counts_check(na.data())) return rc;
            if (int rc = types_check(pair_type ? pt.data() : nullptr)) return rc;
        }
        std::vector<uint32_t> m((size_t)n * A, 0xffffffffu);       // NULL: every template edge (the expansion clears what touches a pad)
        if (mask) fetch(m.data(), mask, m.size() * sizeof(uint32_t));
        S->gt_nat.upload(na); S->gt_mask.upload(m);
        if (pair_type) S->gt_ptype.upload(pt); else S->gt_ptype.release();
        S->g_nat = std::move(na); S->gn = n;
        return TI_OK;
    });
}

}  // extern "C"
