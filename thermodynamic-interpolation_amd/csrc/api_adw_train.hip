// api_adw_train.hip -- the adw trainer of the C ABI (include/ti_hip.h ti_adw_trainer_create .. ti_adw_train_set_lr): the checks, the
// staging, and the launch sequence of a training step -- interpolate (vloss_kernels.hip), forward, loss rows (the velocity loss's own
// reduce kernel), backward, combine, clip + Adam (adw_train_kernels.hip).  A step is enqueued on the handle's stream without a host
// synchronisation: whether it is skipped is decided by the optimiser kernel from the two batch-wide sums in device memory.
// The optimiser shell -- master state, counters, clip + Adam, the state entry points, index handling -- is train_optim.hpp's, shared
// with api_painn_train.hip.
#include "train_optim.hpp"

namespace {

struct TrLayer { int K, N; size_t w_off, b_off; bool act; };      // Linear(K -> N) at its canonical offsets, SiLU behind it or not

struct AdwTrainState : Optim {                  // is_bias: 1 at the bias entries, whose gradients launch_train_bias writes in fp64
    int H = 0, L = 0, dim = 1;
    size_t n_embed = 0;
    std::vector<TrLayer> emb, net;
    DevBuf<double> loss;
    DevBuf<int64_t> idx0, idx1;
    DevBuf<float> part;
    // staged sets of a host call, the gathered minibatch, times, noise, states; activations (y, silu') of every hidden layer, the
    // inputs of both MLPs, the embedding, the drift; the two gradient buffers the backward pass alternates between, the input
    // gradient of net.0, the output gradient of beta_embed
    DevBuf<float> sx0, sx1, sb0, sb1, gx0, gx1, gb0, gb1, t, tin, z, zin, xt, act, e0, a0, embv, bout, ga, gb, ge;
};

AdwTrainState* state_of(ti_handle* h) { return static_cast<AdwTrainState*>(h->train.get()); }

size_t adw_weight_count(int H, int nl, int dim)
{
    return (size_t)H * 3 + H + (size_t)H * H + H + H + 1 + (size_t)H * (dim + 2) + H + (size_t)(nl - 1) * ((size_t)H * H + H) + (size_t)dim * H + dim;
}

// the checks of ti_adw_train_grad / ti_adw_train_steps that need no handle, in the order include/ti_hip.h lists them
int train_call_check(const ti_vloss_desc* d, const float* t, const float* z, int64_t B, int mem)
{
    if (int rc = vloss_check(d, t, z, B, mem)) return rc;
    if (B > TI_ADW_TRAIN_MAX_B) return fail(TI_E_UNSUPPORTED, "B = " + std::to_string(B) + " is above TI_ADW_TRAIN_MAX_B = " + std::to_string(TI_ADW_TRAIN_MAX_B));
    return TI_OK;
}

void ensure_train_ws(AdwTrainState* S, long long B, int halves)
{
    const size_t R = (size_t)halves * B, H = S->H, m = S->dim, K0 = m + 2;
    grow(S->t, (size_t)B); grow(S->z, (size_t)B * m); grow(S->xt, R * m);
    grow(S->act, 2 * ((size_t)2 * B + (size_t)(S->L) * R) * H);        // (y, silu') of beta_embed's two and net's L hidden layers
    grow(S->e0, (size_t)B * 3); grow(S->a0, R * K0); grow(S->embv, (size_t)B); grow(S->bout, R * m);
    grow(S->ga, R * H); grow(S->gb, R * H); grow(S->ge, (size_t)B);
    grow(S->loss, (size_t)B);
    grow(S->part64, (size_t)std::max(vloss_tiles(B), vloss_tiles((long long)S->nW)));
    grow(S->part, (size_t)train_row_tiles((long long)R) * S->nW);
}

// One forward and backward pass on the device-resident rows (x0, x1 [B][m], beta0, beta1 [B]; t, z given or NULL): afterwards S->loss
// holds the loss rows, S->red (their sum, the sum of the squared gradient entries) and S->grad the gradient of the mean loss.
void train_forward_backward(ti_handle* h, AdwTrainState* S, const ti_vloss_desc* d, const float* x0, const float* x1, const float* beta0,
                            const float* beta1, const float* t_given, const float* z_given, long long B, int draw)
{
    hipStream_t st = h->stream;
    const bool two = d->kind == TI_VLOSS_STANDARD;
    const int halves = two ? 2 : 1, m = S->dim, H = S->H, L = S->L;
    const long long R = (long long)halves * B;
    const float* td = t_given;
    if (d->t_dist != TI_TDIST_GIVEN) {
        HIP_CHECK(launch_vloss_draw_t(S->t.p, d->t_dist, d->seed, d->traj_offset, draw, B, st));
        td = S->t.p;
    }
    VlossParams p{};
    p.kind = d->kind; p.gamma = d->gamma; p.center = TI_CENTER_NONE; p.a = d->a;
    p.B = B; p.m = m; p.A = 1;
    p.x0 = x0; p.x1 = x1; p.t = td; p.z_in = z_given;
    p.seed = d->seed; p.traj0 = d->traj_offset; p.draw = draw;
    p.z = two ? S->z.p : nullptr; p.xt = S->xt.p; p.half = B * m;
    HIP_CHECK(launch_vloss_interp(p, st));

    // activations: beta_embed's hidden layers [B][H] first, then net's [R][H]; y and silu' of a layer lie side by side
    float* act = S->act.p;
    auto ey = [&](int l) { return act + (size_t)(2 * l) * B * H; };
    auto ed = [&](int l) { return act + (size_t)(2 * l + 1) * B * H; };
    float* nact = act + (size_t)4 * B * H;
    auto ny = [&](int l) { return nact + (size_t)(2 * l) * R * H; };
    auto nd = [&](int l) { return nact + (size_t)(2 * l + 1) * R * H; };

    auto forward = [&](const TrLayer& ly, const float* in, long long rows, float* y, float* dy) {
        TrGemm g{};
        g.A = in; g.a_si = ly.K; g.a_sk = 1;
        g.B = S->w32.p + ly.w_off; g.b_sk = 1; g.b_sj = ly.K;
        g.M = rows; g.N = ly.N; g.Kd = ly.K; g.ktile = ly.K;
        g.mode = ly.act ? TRG_FWD_ACT : TRG_FWD_LIN;
        g.bias = S->w32.p + ly.b_off; g.out = y; g.out2 = dy; g.ldo = ly.N;
        HIP_CHECK(launch_train_gemm(g, 1, st));
    };
    HIP_CHECK(launch_train_embed_in(S->e0.p, beta0, beta1, td, B, st));
    forward(S->emb[0], S->e0.p, B, ey(0), ed(0));
    forward(S->emb[1], ey(0), B, ey(1), ed(1));
    forward(S->emb[2], ey(1), B, S->embv.p, nullptr);
    HIP_CHECK(launch_train_net_in(S->a0.p, S->xt.p, td, S->embv.p, B, halves, m, st));
    for (int l = 0; l <= L; ++l)
        forward(S->net[l], l == 0 ? S->a0.p : ny(l - 1), R, l < L ? ny(l) : S->bout.p, l < L ? nd(l) : nullptr);

    // the loss rows by the velocity loss's own kernel, their sum by its fixed tree
    p.b = S->bout.p; p.loss = S->loss.p;
    HIP_CHECK(launch_vloss_reduce(p, st));
    HIP_CHECK(launch_vloss_colsum(S->red.p + RED_LOSS, S->part64.p, S->loss.p, B, 1, st));

    // backward: gz of a layer in `cur`, the layer in front of it gets `nxt`
    float *cur = S->ga.p, *nxt = S->gb.p;
    HIP_CHECK(launch_train_gout(cur, p, st));
    const int tiles_n = (int)train_row_tiles(R), tiles_e = (int)train_row_tiles(B);
    auto wgrad = [&](const TrLayer& ly, const float* gz, const float* in, long long rows, int tiles) {
        TrGemm g{};
        g.A = gz; g.a_si = 1; g.a_sk = ly.N;
        g.B = in; g.b_sk = ly.K; g.b_sj = 1;
        g.M = ly.N; g.N = ly.K; g.Kd = rows; g.ktile = TRAIN_ROW_TILE;
        g.mode = TRG_WGRAD;
        g.part = S->part.p; g.part_stride = S->nW; g.w_off = ly.w_off; g.Kin = ly.K;
        HIP_CHECK(launch_train_gemm(g, tiles, st));
        HIP_CHECK(launch_train_bias(S->grad.p + ly.b_off, gz, rows, ly.N, st));
    };
    auto backward = [&](const TrLayer& ly, const float* gz, long long rows, const float* dact, float* out) {
        TrGemm g{};
        g.A = gz; g.a_si = ly.N; g.a_sk = 1;
        g.B = S->w32.p + ly.w_off; g.b_sk = ly.K; g.b_sj = 1;
        g.M = rows; g.N = ly.K; g.Kd = ly.N; g.ktile = ly.N;
        g.mode = dact ? TRG_BWD_ACT : TRG_BWD_LIN;
        g.dact = dact; g.out = out; g.ldo = ly.K;
        HIP_CHECK(launch_train_gemm(g, 1, st));
    };
    for (int l = L; l >= 0; --l) {
        wgrad(S->net[l], cur, l == 0 ? S->a0.p : ny(l - 1), R, tiles_n);
        if (l > 0) { backward(S->net[l], cur, R, nd(l - 1), nxt); std::swap(cur, nxt); }
    }
    // of net.0's input gradient only the embedding column is needed: it goes to beta_embed
    HIP_CHECK(launch_train_embed_gout(S->ge.p, cur, S->w32.p + S->net[0].w_off, B, halves, H, m + 2, st));
    std::swap(cur, nxt);                          // gz of net.0 has been read by then (stream order); `cur` is free again
    wgrad(S->emb[2], S->ge.p, ey(1), B, tiles_e);
    backward(S->emb[2], S->ge.p, B, ed(1), cur);
    wgrad(S->emb[1], cur, ey(0), B, tiles_e);
    backward(S->emb[1], cur, B, ed(0), nxt);
    wgrad(S->emb[0], nxt, S->e0.p, B, tiles_e);

    HIP_CHECK(launch_train_combine(S->grad.p, S->sq.p, S->part.p, S->is_bias.p, S->nW, S->nW, S->n_embed, tiles_e, tiles_n, st));
    HIP_CHECK(launch_vloss_colsum(S->red.p + RED_SUMSQ, S->part64.p, S->sq.p, (long long)S->nW, 1, st));
}

}  // namespace

extern "C" {

ti_handle* ti_adw_trainer_create(const ti_adw_desc* d, int32_t dim, const double* weights, size_t n_weights, const ti_adw_train_desc* td,
                                 int device)
{
    ti_handle* out = nullptr;
    const int rc = guarded([&]() -> int {
        if (!d || !weights) return fail(TI_E_ARG, "NULL argument");
        if (dim < 1 || dim > 16) return fail(TI_E_UNSUPPORTED, "dim must be 1..16 (FCNetMultiBeta(d, d, H, L)), got " + std::to_string(dim));
        const int H = d->hidden_size, nl = d->num_layers;
        if (H != 32 && H != 64 && H != 128 && H != 256) return fail(TI_E_UNSUPPORTED, "hidden_size must be 32, 64, 128 or 256");
        if (nl < 1) return fail(TI_E_ARG, "num_layers must be >= 1");
        if (d->precision != TI_PREC_F32 && d->precision != TI_PREC_F16X2) return fail(TI_E_ARG, "unknown precision");
        if (d->precision != TI_PREC_F32) return fail(TI_E_UNSUPPORTED, "the trainer takes TI_PREC_F32 only");
        const size_t need = adw_weight_count(H, nl, dim);
        if (n_weights != need) return fail(TI_E_ARG, "weight count mismatch: expected " + std::to_string(need) + ", got " + std::to_string(n_weights));
        if (!td) return fail(TI_E_ARG, "train desc is NULL");
        const AdamDesc ad{td->lr, td->beta1, td->beta2, td->eps, td->weight_decay, td->max_grad_norm};
        if (int rc2 = adam_desc_check(ad)) return rc2;
        std::unique_ptr<ti_handle> h(new_handle(2, device));
        h->ad = *d; h->NB = H / 32; h->a_dim = dim;
        auto S = std::make_shared<AdwTrainState>();
        S->H = H; S->L = nl; S->dim = dim;
        size_t o = 0;
        auto take = [&](std::vector<TrLayer>& v, int K, int N, bool act) {
            v.push_back(TrLayer{K, N, o, o + (size_t)N * K, act});
            o += (size_t)N * K + N;
        };
        take(S->emb, 3, H, true); take(S->emb, H, H, true); take(S->emb, H, 1, false);
        S->n_embed = o;
        take(S->net, dim + 2, H, true);
        for (int l = 1; l < nl; ++l) take(S->net, H, H, true);
        take(S->net, H, dim, false);
        std::vector<unsigned char> mask(need, 0);
        for (const auto* v : {&S->emb, &S->net})
            for (const TrLayer& ly : *v) std::fill(mask.begin() + ly.b_off, mask.begin() + ly.b_off + ly.N, (unsigned char)1);
        S->setup(ad, weights, mask, 2, 0, h->stream);
        h->train = S;
        out = h.release();
        return TI_OK;
    });
    return rc == TI_OK ? out : nullptr;
}

int ti_adw_train_grad(ti_handle* h, const ti_vloss_desc* d, const float* x0, const float* x1, const float* beta0, const float* beta1,
                      const float* t, const float* z, int64_t B, double* out_loss, double* out_mean, double* out_grad, double* out_gnorm, int mem)
{
    if (int rc = train_call_check(d, t, z, B, mem)) return rc;
    if (!x0 || !x1 || !beta0 || !beta1) return fail(TI_E_ARG, "NULL buffer");
    if (d->center != TI_CENTER_NONE) return fail(TI_E_UNSUPPORTED, "an adw trainer takes TI_CENTER_NONE only");
    if (!h || h->kind != 2) return fail(TI_E_ARG, "not an adw trainer handle");
    return guarded([&]() -> int {
        set_device(h);
        AdwTrainState* S = state_of(h);
        Staged sg(h, mem);
        const size_t n = (size_t)B * S->dim;
        ensure_train_ws(S, B, d->kind == TI_VLOSS_STANDARD ? 2 : 1);
        const float *x0d = sg.in(x0, S->sx0, n), *x1d = sg.in(x1, S->sx1, n);
        const float *b0d = sg.in(beta0, S->sb0, (size_t)B), *b1d = sg.in(beta1, S->sb1, (size_t)B);
        const float *td = sg.in(t, S->tin, (size_t)B), *zd = sg.in(z, S->zin, n);
        train_forward_backward(h, S, d, x0d, x1d, b0d, b1d, td, zd, B, d->draw);
        return S->grad_readback(out_loss, out_mean, out_grad, out_gnorm, B, (double)B, mem, S->loss.p, h->stream);
    });
}

int ti_adw_train_apply(ti_handle* h, const double* grad, int32_t* out_skipped)
{
    if (!grad) return fail(TI_E_ARG, "NULL buffer");
    if (!h || h->kind != 2) return fail(TI_E_ARG, "not an adw trainer handle");
    return guarded([&]() -> int { set_device(h); return state_of(h)->apply(grad, out_skipped, state_of(h)->n_embed, h->stream); });
}

int ti_adw_train_steps(ti_handle* h, const ti_vloss_desc* d, const float* x0, int64_t n0, const float* x1, int64_t n1, const float* beta0,
                       const float* beta1, const int64_t* idx0, const int64_t* idx1, const float* t, const float* z, int64_t B,
                       int64_t n_steps, double* out_loss, int64_t* out_skipped, int mem)
{
    if (int rc = train_call_check(d, t, z, B, mem)) return rc;
    if (n_steps < 1 || n_steps > INT32_MAX) return fail(TI_E_ARG, "n_steps must be in 1..2^31 - 1");
    if ((idx0 == nullptr) != (idx1 == nullptr)) return fail(TI_E_ARG, "idx0 and idx1 must both be given or both be NULL");
    if (!idx0 && n_steps != 1) return fail(TI_E_ARG, "without indices n_steps must be 1");
    if ((t || z) && n_steps != 1) return fail(TI_E_ARG, "a given t or z needs n_steps == 1");
    if (n0 < 1 || n1 < 1 || (!idx0 && (n0 < B || n1 < B))) return fail(TI_E_ARG, "n0 / n1 do not cover the rows of a step");
    if ((long long)d->draw + (n_steps - 1) > INT32_MAX) return fail(TI_E_ARG, "draw + n_steps overflows the draw index");
    if (!x0 || !x1 || !beta0 || !beta1) return fail(TI_E_ARG, "NULL buffer");
    if (d->center != TI_CENTER_NONE) return fail(TI_E_UNSUPPORTED, "an adw trainer takes TI_CENTER_NONE only");
    const size_t n_idx = idx0 ? (size_t)n_steps * (size_t)B : 0;
    if (idx0 && mem == TI_MEM_HOST) if (int rc = train_idx_check(idx0, idx1, n_idx, n0, n1, true, mem)) return rc;
    if (!h || h->kind != 2) return fail(TI_E_ARG, "not an adw trainer handle");
    return guarded([&]() -> int {
        set_device(h);
        AdwTrainState* S = state_of(h);
        hipStream_t st = h->stream;
        Staged sg(h, mem);
        const int m = S->dim;
        if (idx0 && !sg.host) if (int rc = train_idx_check(idx0, idx1, n_idx, n0, n1, true, mem)) return rc;      // nothing has been enqueued yet
        ensure_train_ws(S, B, d->kind == TI_VLOSS_STANDARD ? 2 : 1);
        grow(S->log, (size_t)n_steps);
        const float *x0d = sg.in(x0, S->sx0, (size_t)n0 * m), *x1d = sg.in(x1, S->sx1, (size_t)n1 * m);
        const float *b0d = sg.in(beta0, S->sb0, (size_t)n0), *b1d = sg.in(beta1, S->sb1, (size_t)n1);
        const float *td = sg.in(t, S->tin, (size_t)B), *zd = sg.in(z, S->zin, (size_t)B * m);
        const long long *i0d = idx_ll(sg.in(idx0, S->idx0, n_idx)), *i1d = idx_ll(sg.in(idx1, S->idx1, n_idx));
        if (idx0) { grow(S->gx0, (size_t)B * m); grow(S->gx1, (size_t)B * m); grow(S->gb0, (size_t)B); grow(S->gb1, (size_t)B); }
        S->read_counters(st);                 // as in ti_adw_train_apply: bias and log are indexed from these
        S->upload_bias(n_steps, st);
        const TrAdam a = S->adam_params(true, (double)B, S->log.p);
        for (int64_t k = 0; k < n_steps; ++k) {
            const float *xa = x0d, *xb = x1d, *ba = b0d, *bb = b1d;
            if (idx0) {
                HIP_CHECK(launch_train_gather(S->gx0.p, x0d, i0d + k * B, n0, B, m, st));
                HIP_CHECK(launch_train_gather(S->gx1.p, x1d, i1d + k * B, n1, B, m, st));
                HIP_CHECK(launch_train_gather(S->gb0.p, b0d, i0d + k * B, n0, B, 1, st));
                HIP_CHECK(launch_train_gather(S->gb1.p, b1d, i1d + k * B, n1, B, 1, st));
                xa = S->gx0.p; xb = S->gx1.p; ba = S->gb0.p; bb = S->gb1.p;
            }
            train_forward_backward(h, S, d, xa, xb, ba, bb, td, zd, B, d->draw + (int)k);
            HIP_CHECK(launch_train_adam(a, st));
            HIP_CHECK(launch_train_finish(a, st));
        }
        S->steps_readback(out_loss, out_skipped, n_steps, st);
        return TI_OK;
    });
}

int ti_adw_train_get_state(ti_handle* h, double* w, double* m, double* v, int64_t* n_applied, int64_t* n_skipped)
{
    if (!h || h->kind != 2) return fail(TI_E_ARG, "not an adw trainer handle");
    return guarded([&]() -> int { set_device(h); return state_of(h)->get_state(w, m, v, n_applied, n_skipped, h->stream); });
}

int ti_adw_train_set_state(ti_handle* h, const double* w, const double* m, const double* v, int64_t n_applied)
{
    if (n_applied < 0) return fail(TI_E_ARG, "n_applied < 0");
    if (!h || h->kind != 2) return fail(TI_E_ARG, "not an adw trainer handle");
    return guarded([&]() -> int { set_device(h); return state_of(h)->set_state(w, m, v, n_applied, h->stream); });
}

int ti_adw_train_set_lr(ti_handle* h, double lr)
{
    if (int rc = lr_check(lr)) return rc;
    if (!h || h->kind != 2) return fail(TI_E_ARG, "not an adw trainer handle");
    state_of(h)->td.lr = lr;
    return TI_OK;
}

}  // extern "C"
