// api_adw.hip -- the adw (FCNetMultiBeta) entry points of the C ABI (include/ti_hip.h): creation, drift, rollouts, the fused rollout.
#include "rollout.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ adw helpers
void adw_mlp_launch(ti_handle* h, bool embed, const float* a0, const float* in1, const float* emb, const int32_t* idx, float t,
                    long long rows, float* out, float* out_div)
{
    AdwParams p{};
    const Stream& s2 = embed ? h->st_be : h->st_net;
    p.stream = h->S(s2); p.nch = s2.nch;
    p.vecs = h->F(embed ? h->a_be_vecs : h->a_net_vecs);
    p.b_out = embed ? h->a_be_b_out : h->a_b_out; p.n_hidden = embed ? 1 : h->ad.num_layers - 1; p.B = rows;
    p.x = a0; p.in1 = in1; p.emb = emb; p.idx = idx; p.t = t; p.out = out; p.out_div = out_div;
    p.dim = embed ? 1 : h->a_dim;
    Timed tm(h, TI_KERNEL_ADW);
    HIP_CHECK(launch_adw(h->NB, h->ad.precision == TI_PREC_F16X2, p, h->stream));
}

// upload conditioning: dedupe (beta0, beta1) pairs on the host (the driver uses one pair, adw/sample.py:24)
long long adw_set_cond(ti_handle* h, const float* beta0, const float* beta1, long long B, int mem, std::vector<float>* u0_out = nullptr,
                       std::vector<float>* u1_out = nullptr)
{
    std::vector<float> b0(B), b1(B);
    if (mem == TI_MEM_DEVICE) {
        HIP_CHECK(hipMemcpy(b0.data(), beta0, B * sizeof(float), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(b1.data(), beta1, B * sizeof(float), hipMemcpyDeviceToHost));
    } else { std::memcpy(b0.data(), beta0, B * sizeof(float)); std::memcpy(b1.data(), beta1, B * sizeof(float)); }
    std::map<std::pair<float, float>, int> uniq;
    std::vector<int32_t> idx(B);
    std::vector<float> u0, u1;
    for (long long i = 0; i < B; ++i) {
        auto key = std::make_pair(b0[i], b1[i]);
        auto it = uniq.find(key);
        if (it == uniq.end()) { it = uniq.emplace(key, (int)u0.size()).first; u0.push_back(b0[i]); u1.push_back(b1[i]); }
        idx[i] = it->second;
    }
    h->aidx.upload(idx); h->abeta0_u.upload(u0); h->abeta1_u.upload(u1);
    h->aemb_u.alloc(u0.size());
    if (u0_out) *u0_out = u0;
    if (u1_out) *u1_out = u1;
    return (long long)u0.size();
}

// out_div (may be NULL): sum_i d b_i / d x_i, the divergence of the drift (beta_embed does not depend on x); x / out [B][d]
void adw_drift_dev(ti_handle* h, const float* x_dev, float t, long long U, long long B, float* out_dev, float* out_div)
{
    adw_mlp_launch(h, true, h->abeta0_u.p, h->abeta1_u.p, nullptr, nullptr, t, U, h->aemb_u.p, nullptr);   // beta_embed([b0, b1, t])
    adw_mlp_launch(h, false, x_dev, nullptr, h->aemb_u.p, h->aidx.p, t, B, out_dev, out_div);             // net([x, t, embed])
}

}  // namespace

namespace ti {

// per-row times: beta_embed([b0_i, b1_i, t_i]) per row (no dedupe: the time differs per row), then net([x_i, t_i, emb_i]).
// beta0 / beta1 / tv are device pointers [B].
void adw_drift_tv_dev(ti_handle* h, const float* x_dev, const float* tv, const float* beta0, const float* beta1, long long B, float* out_dev,
                      float* out_div)
{
    grow(h->aemb_r, (size_t)B);
    adw_mlp_launch(h, true, beta0, beta1, tv, nullptr, 0.f, B, h->aemb_r.p, nullptr);          // a2 = emb[r] = t_r
    adw_mlp_launch(h, false, x_dev, tv, h->aemb_r.p, nullptr, 0.f, B, out_dev, out_div);       // a1 = in1[r] = t_r
}

void ensure_adw_ws(ti_handle* h, long long B)
{
    if (B <= h->cap) return;
    const size_t n = (size_t)B * h->a_dim;             // state floats; the divergence / dlogp buffers hold one per particle
    h->ax.alloc(n); h->ab1.alloc(n); h->ab2.alloc(n); h->axt.alloc(n); h->adl.alloc(B); h->ad1.alloc(B); h->ad2.alloc(B);
    h->cap = B;
}

}  // namespace ti

extern "C" {

ti_handle* ti_adw_create(const ti_adw_desc* d, const double* weights, size_t n_weights, int device)
{
    return ti_adw_create_nd(d, 1, weights, n_weights, device);
}

ti_handle* ti_adw_create_nd(const ti_adw_desc* d, int32_t dim, const double* weights, size_t n_weights, int device)
{
    ti_handle* out = nullptr;
    const int rc = guarded([&]() -> int {
        if (!d || !weights) return fail(TI_E_ARG, "NULL argument");
        if (dim < 1 || dim > 16) return fail(TI_E_UNSUPPORTED, "dim must be 1..16 (FCNetMultiBeta(d, d, H, L)), got " + std::to_string(dim));
        const int H = d->hidden_size, nl = d->num_layers;
        if (H != 32 && H != 64 && H != 128 && H != 256) return fail(TI_E_UNSUPPORTED, "hidden_size must be 32, 64, 128 or 256");
        if (nl < 1) return fail(TI_E_ARG, "num_layers must be >= 1");
        if (d->precision != TI_PREC_F32 && d->precision != TI_PREC_F16X2) return fail(TI_E_ARG, "unknown precision");
        const size_t need = (size_t)H * 3 + H + (size_t)H * H + H + H + 1 + (size_t)H * (dim + 2) + H + (size_t)(nl - 1) * ((size_t)H * H + H) +
                            (size_t)dim * H + dim;
        if (n_weights != need) return fail(TI_E_ARG, "weight count mismatch: expected " + std::to_string(need) + ", got " + std::to_string(n_weights));
        if (d->precision == TI_PREC_F16X2)          // the weights' hi halves are plain fp16: refuse what would round to inf
            for (size_t i = 0; i < n_weights; ++i)
                if (!(std::fabs(weights[i]) < 65504.0))
                    return fail(TI_E_UNSUPPORTED, "precision f16x2 needs every weight to be finite and below 65504 in magnitude (weight " + std::to_string(i) + ")");
        std::unique_ptr<ti_handle> h(new_handle(1, device));
        h->ad = *d; h->NB = H / 32; h->a_dim = dim;
        std::vector<float> w(n_weights);
        for (size_t i = 0; i < n_weights; ++i) w[i] = (float)weights[i];        // the device computes in fp32
        const int NB = h->NB, NBK = H / 16;
        const bool split = d->precision == TI_PREC_F16X2;
        std::vector<float> nat, pk;
        auto chunk16 = [&](const float* W, int row0) {
            if (split) pack_chunk16_split(pk, W, H, H, row0, 0, NBK); else pack_chunk16(pk, W, H, H, row0, 0, NBK);
        };
        // one MLP block: canonical order  W_in[H,K] b_in[H] (W_h[H,H] b_h[H]) x n_hidden  W_out[D,H] b_out[D]  (K = D + 2)
        // D = 1: vector block w_in [H][3] | b_in | b_hidden | w_out, b_out a kernel argument.  D > 1: w_in [H][Kpad] (zero
        // columns up to a multiple of 4) | b_in | b_hidden | w_out [D][H] | b_out [D] (zeros up to a multiple of 4).
        auto take_mlp = [&](size_t& o, int n_hidden, size_t& vec_off, Stream& st, float& b_out, int D) {
            vec_off = nat.size();
            const int K = D + 2, Kpad = D == 1 ? 3 : (K + 3) / 4 * 4;
            for (int f = 0; f < H; ++f) {                                               // w_in
                nat.insert(nat.end(), &w[o + (size_t)f * K], &w[o + (size_t)f * K] + K);
                nat.insert(nat.end(), (size_t)(Kpad - K), 0.f);
            }
            o += (size_t)H * K;
            nat.insert(nat.end(), &w[o], &w[o] + H); o += H;                              // b_in
            st.off4 = pk.size() / 4;
            std::vector<float> bh;
            for (int l = 0; l < n_hidden; ++l) {
                for (int nbo = 0; nbo < NB; ++nbo) chunk16(&w[o], 32 * nbo);
                o += (size_t)H * H;
                bh.insert(bh.end(), &w[o], &w[o] + H); o += H;
            }
            st.nch = n_hidden * NB;
            nat.insert(nat.end(), bh.begin(), bh.end());
            nat.insert(nat.end(), &w[o], &w[o] + (size_t)D * H); o += (size_t)D * H;      // w_out
            if (D == 1) { b_out = w[o]; o += 1; return; }
            nat.insert(nat.end(), &w[o], &w[o] + D); o += D;                               // b_out
            nat.insert(nat.end(), (size_t)((D + 3) / 4 * 4 - D), 0.f);
            b_out = 0.f;
        };
        size_t o = 0;
        take_mlp(o, 1, h->a_be_vecs, h->st_be, h->a_be_b_out, 1);
        take_mlp(o, nl - 1, h->a_net_vecs, h->st_net, h->a_b_out, dim);
        if (pk.empty()) pk.assign(4, 0.f);
        h->flat.upload(nat); h->packed.upload(pk);
        HIP_CHECK(configure_adw_kernels(NB, std::max(1, nl - 1), dim));
        if (dim == 1) HIP_CHECK(configure_adw_fused_kernels(NB, std::max(1, nl - 1)));
        out = h.release();
        return TI_OK;
    });
    return rc == TI_OK ? out : nullptr;
}

// ti_adw_drift / ti_adw_drift_div (one time t; out_div may be NULL) and ti_adw_drift_tv (per_row_t: tv [B] holds one time per row)
static int adw_drift_impl(ti_handle* h, const float* x, float t, const float* tv, bool per_row_t, const float* beta0, const float* beta1,
                          int64_t B, float* out, float* out_div, int mem)
{
    if (!h || h->kind != 1) return fail(TI_E_ARG, "not an adw handle");
    if (B < 0 || (B > 0 && (!x || (per_row_t && !tv) || !beta0 || !beta1 || !out))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        ensure_adw_ws(h, B);
        Staged sg(h, mem);
        // one time: the distinct (beta0, beta1) pairs, deduplicated on the host; per-row times: the rows as they are
        const long long U = per_row_t ? 0 : adw_set_cond(h, beta0, beta1, B, mem);
        const float* b0d = per_row_t ? sg.in(beta0, h->abeta0_r, (size_t)B) : nullptr;
        const float* b1d = per_row_t ? sg.in(beta1, h->abeta1_r, (size_t)B) : nullptr;
        const size_t n = (size_t)B * h->a_dim;
        const float* xd = sg.in(x, h->ax, n);
        const float* td = per_row_t ? sg.in(tv, h->atv, (size_t)B) : nullptr;
        float* od = sg.out(out, h->ab1, n);
        float* dd = out_div ? sg.out(out_div, h->ad1, (size_t)B) : nullptr;
        if (per_row_t) adw_drift_tv_dev(h, xd, td, b0d, b1d, B, od, dd);
        else adw_drift_dev(h, xd, t, U, B, od, dd);
        sg.finish();
        return TI_OK;
    });
}

int ti_adw_drift(ti_handle* h, const float* x, float t, const float* beta0, const float* beta1, int64_t B, float* out, int mem)
{
    return adw_drift_impl(h, x, t, nullptr, false, beta0, beta1, B, out, nullptr, mem);
}

int ti_adw_drift_div(ti_handle* h, const float* x, float t, const float* beta0, const float* beta1, int64_t B, float* out, float* out_div, int mem)
{
    if (!out_div) return fail(TI_E_ARG, "out_div is NULL");
    return adw_drift_impl(h, x, t, nullptr, false, beta0, beta1, B, out, out_div, mem);
}

int ti_adw_drift_tv(ti_handle* h, const float* x, const float* t, const float* beta0, const float* beta1, int64_t B, float* out,
                    float* out_div, int mem)
{
    return adw_drift_impl(h, x, 0.f, t, true, beta0, beta1, B, out, out_div, mem);
}

static int adw_rollout_impl(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* beta0, const float* beta1, int64_t B,
                            float* out_path, float* out_dlogp, int64_t* n_fevals)
{
    if (!h || h->kind != 1) return fail(TI_E_ARG, "not an adw handle");
    if (int rc = check_rollout_desc(rd)) return rc;
    if (rd->scheme == TI_SCHEME_DOPRI5_TRAJ && h->obs[1].K > 0) return fail(TI_E_UNSUPPORTED, MSG_TRAJ_OBSERVER);
    if (B < 0 || (B > 0 && (!x0 || !beta0 || !beta1 || !out_path))) return fail(TI_E_ARG, "NULL buffer");
    if (out_dlogp && rd->scheme == TI_SCHEME_EM && rd->eps > 0.f) return fail(TI_E_UNSUPPORTED, MSG_EM_DLOGP);
    if (B == 0) { if (n_fevals) *n_fevals = 0; return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        ensure_adw_ws(h, B);
        const long long U = adw_set_cond(h, beta0, beta1, B, rd->mem);
        const hipMemcpyKind in_kind = rd->mem == TI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        const int D = h->a_dim;
        const size_t n = (size_t)B * D;
        HIP_CHECK(hipMemcpyAsync(h->ax.p, x0, n * sizeof(float), in_kind, h->stream));
        DlogpAux aux;
        aux.n_dl = (size_t)B;                        // one dlogp entry per particle
        DevBuf<float> scaled_tmp;                    // dlogp * 1e2 staging for the saved rows
        if (out_dlogp) { scaled_tmp.alloc(B); aux.dl = h->adl.p; aux.d1 = h->ad1.p; aux.d2 = h->ad2.p; aux.scaled = scaled_tmp.p; aux.out = out_dlogp; }
        auto drift = [&](const float* xs, float t, float* o, float* dv) { adw_drift_dev(h, xs, t, U, B, o, dv); };
        if (rd->scheme == TI_SCHEME_DOPRI5_TRAJ) {
            Staged sg(h, rd->mem);      // per-row conditioning: the rows as they are
            const float *b0d = sg.in(beta0, h->abeta0_r, (size_t)B), *b1d = sg.in(beta1, h->abeta1_r, (size_t)B);
            auto drift_tv = [&](const float* xs, const float* tv, float* o, float* dv) { adw_drift_tv_dev(h, xs, tv, b0d, b1d, B, o, dv); };
            return rollout_rk_traj(h, rd, h->ax.p, B, D, out_path, n_fevals, drift_tv, aux);
        }
        if (rd->scheme >= TI_SCHEME_DOPRI5) return rollout_rk(h, rd, h->ax.p, n, out_path, n_fevals, drift, aux);
        return rollout_common(h, rd, h->ax.p, h->ab1.p, h->ab2.p, h->axt.p, n, B, D, 0, out_path, n_fevals, drift, aux);
    });
}

int ti_adw_rollout(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* beta0, const float* beta1, int64_t B,
                   float* out_path, int64_t* n_fevals)
{
    return adw_rollout_impl(h, rd, x0, beta0, beta1, B, out_path, nullptr, n_fevals);
}

int ti_adw_rollout_dlogp(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* beta0, const float* beta1, int64_t B,
                         float* out_path, float* out_dlogp, int64_t* n_fevals)
{
    if (!out_dlogp) return fail(TI_E_ARG, "out_dlogp is NULL");
    return adw_rollout_impl(h, rd, x0, beta0, beta1, B, out_path, out_dlogp, n_fevals);
}

// A whole Euler / Heun / EM rollout of a 1-D handle in two launches: the beta-embedding table of every grid point (the embedding
// kernel in its per-row-time mode over n_step * U rows) and adw_rollout_fused_kernel.  Every per-step scalar is computed here with the
// fp32 expressions of rollout_common; the kernel applies them with the roundings of axpy_kernel / heun_kernel / noise_kernel /
// scale_kernel, so the result is that of ti_adw_rollout(_dlogp) bit for bit.
int ti_adw_rollout_fused(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* beta0, const float* beta1, int64_t B,
                         float* out_path, float* out_dlogp, int64_t* n_fevals)
{
    if (!h || h->kind != 1) return fail(TI_E_ARG, "not an adw handle");
    if (int rc = check_rollout_desc(rd)) return rc;
    if (h->a_dim > 1) return fail(TI_E_UNSUPPORTED, "the fused rollout covers 1-D handles: use ti_adw_rollout for dim = " + std::to_string(h->a_dim));
    if (rd->scheme != TI_SCHEME_EULER && rd->scheme != TI_SCHEME_HEUN && rd->scheme != TI_SCHEME_EM)
        return fail(TI_E_UNSUPPORTED, "the fused rollout covers the Euler, Heun and EM schemes: use ti_adw_rollout for the others");
    if (h->obs[1].K > 0)
        return fail(TI_E_UNSUPPORTED, "the fused rollout writes its rows inside a kernel: detach the observer (ti_obs_set_observer)");
    if (B < 0 || (B > 0 && (!x0 || !beta0 || !beta1 || !out_path))) return fail(TI_E_ARG, "NULL buffer");
    if (out_dlogp && rd->scheme == TI_SCHEME_EM && rd->eps > 0.f) return fail(TI_E_UNSUPPORTED, MSG_EM_DLOGP);
    if (B == 0) { if (n_fevals) *n_fevals = 0; return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        ensure_adw_ws(h, B);
        std::vector<float> u0, u1;
        const long long U = adw_set_cond(h, beta0, beta1, B, rd->mem, &u0, &u1);
        const int N = rd->n_step;
        if ((long long)N * U > (1LL << 24))
            return fail(TI_E_UNSUPPORTED, "the fused rollout's embedding table is limited to 2^24 rows, n_step * distinct (beta0, beta1) pairs = " +
                                              std::to_string((long long)N * U) + ": use ti_adw_rollout");
        hipStream_t st = h->stream;
        const bool dev = rd->mem == TI_MEM_DEVICE;
        HIP_CHECK(hipMemcpyAsync(h->ax.p, x0, (size_t)B * sizeof(float), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        // beta embedding at every grid point, rows (k, u): one launch of the embedding kernel with one time per row
        const size_t nt = (size_t)N * U;
        std::vector<float> tb0(nt), tb1(nt), ttv(nt);
        for (int k = 0; k < N; ++k)
            for (long long u = 0; u < U; ++u) { tb0[k * U + u] = u0[u]; tb1[k * U + u] = u1[u]; ttv[k * U + u] = rd->t_grid[k]; }
        // (the host vectors of this call outlive the stream synchronisation at its end)
        grow(h->af_b0, nt); grow(h->af_b1, nt); grow(h->af_tv, nt); grow(h->af_emb, nt);
        HIP_CHECK(hipMemcpyAsync(h->af_b0.p, tb0.data(), nt * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(h->af_b1.p, tb1.data(), nt * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(h->af_tv.p, ttv.data(), nt * sizeof(float), hipMemcpyHostToDevice, st));
        adw_mlp_launch(h, true, h->af_b0.p, h->af_b1.p, h->af_tv.p, nullptr, 0.f, (long long)nt, h->af_emb.p, nullptr);
        // per-step scalars: the expressions of rollout_common, in fp32
        const DlogpAux aux;
        const bool noise = rd->scheme == TI_SCHEME_EM && rd->eps > 0.0f;
        std::vector<AdwFusedStep> steps(std::max(N - 1, 1));
        for (int k = 0; k < N - 1; ++k) {
            const float dt = rd->t_grid[k + 1] - rd->t_grid[k];
            AdwFusedStep& s = steps[k];
            s.t = rd->t_grid[k]; s.t_next = rd->t_grid[k + 1];
            s.dt = dt; s.hdt = 0.5f * dt;
            s.ndt = -dt * aux.div_scale; s.nhdt = -0.5f * dt * aux.div_scale;
            s.sigma = noise ? std::sqrt(2.0f * rd->eps * std::fabs(dt)) : 0.0f;
            s.pad = 0.0f;
        }
        grow(h->af_steps, steps.size());
        HIP_CHECK(hipMemcpyAsync(h->af_steps.p, steps.data(), steps.size() * sizeof(AdwFusedStep), hipMemcpyHostToDevice, st));
        const size_t rows = (size_t)ti_rollout_rows(N, rd->save_every), nout = rows * (size_t)B;
        float *pd = out_path, *dd = out_dlogp;
        if (!dev) {
            grow(h->af_path, nout);
            pd = h->af_path.p;
            if (out_dlogp) { grow(h->af_dl, nout); dd = h->af_dl.p; }
        }
        AdwFusedParams p{};
        p.stream = h->S(h->st_net); p.nch = h->st_net.nch; p.vecs = h->F(h->a_net_vecs); p.b_out = h->a_b_out;
        p.n_hidden = h->ad.num_layers - 1; p.B = B;
        p.x = h->ax.p; p.idx = h->aidx.p; p.emb = h->af_emb.p; p.U = U; p.steps = h->af_steps.p;
        p.n_step = N; p.save_every = rd->save_every;
        p.scheme = rd->scheme == TI_SCHEME_HEUN ? ADW_FUSED_HEUN : noise ? ADW_FUSED_EM : ADW_FUSED_EULER;
        p.seed = rd->seed; p.traj0 = rd->traj_offset; p.step0 = (int)rd->step_offset;
        p.out_path = pd; p.out_dlogp = dd; p.out_scale = aux.out_scale;
        {
            Timed tm(h, TI_KERNEL_ADW);
            HIP_CHECK(launch_adw_fused(h->NB, h->ad.precision == TI_PREC_F16X2, p, st));
        }
        if (!dev) {
            HIP_CHECK(hipMemcpyAsync(out_path, pd, nout * sizeof(float), hipMemcpyDeviceToHost, st));
            if (out_dlogp) HIP_CHECK(hipMemcpyAsync(out_dlogp, dd, nout * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        if (n_fevals) *n_fevals = (int64_t)(N - 1) * (rd->scheme == TI_SCHEME_HEUN ? 2 : 1);
        return final_state_check(h, h->ax.p, (size_t)B);
    });
}

}  // extern "C"
