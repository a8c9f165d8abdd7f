// api_vloss.hip -- the velocity loss of the C ABI (include/ti_hip.h ti_painn_vloss, ti_adw_vloss and their _interp twins): the checks,
// the staging, and the three stages -- interpolate (vloss_kernels.hip), one evaluation of the per-molecule-time drift on the
// device-resident states, reduce.  Every stage computes into buffers of the handle; the outputs are copied from them once the whole
// call has succeeded.
#include "ti_handle.hpp"
#include "adw_train.hpp"

namespace {

constexpr int RED_COLSUM = 0, RED_MEAN = 32, RED_BAD = 33, RED_TBINS = 34;      // slots of ti_handle::vl_red

}  // namespace

// The checks that need no handle, in the order include/ti_hip.h lists them; the handle is refused after them, so that each can be
// exercised without a device.  The adw trainer (api_adw_train.hip) makes the same checks first.
int ti::vloss_check(const ti_vloss_desc* d, const float* t, const float* z, int64_t B, int mem)
{
    if (!d) return fail(TI_E_ARG, "desc is NULL");
    if (d->kind != TI_VLOSS_STANDARD && d->kind != TI_VLOSS_ONE_SIDED) return fail(TI_E_ARG, "unknown loss kind " + std::to_string(d->kind));
    if (d->gamma < TI_GAMMA_BROWNIAN || d->gamma > TI_GAMMA_SIG_SUM) return fail(TI_E_ARG, "unknown gamma kind " + std::to_string(d->gamma));
    if (d->center < TI_CENTER_BATCH || d->center > TI_CENTER_NONE) return fail(TI_E_ARG, "unknown center mode " + std::to_string(d->center));
    if (d->t_dist < TI_TDIST_GIVEN || d->t_dist > TI_TDIST_BETA_2_1) return fail(TI_E_ARG, "unknown time distribution " + std::to_string(d->t_dist));
    const bool two = d->kind == TI_VLOSS_STANDARD;
    if (two && d->gamma != TI_GAMMA_SIN2 && !(std::isfinite(d->a) && d->a > 0.0)) return fail(TI_E_ARG, "gamma's parameter a must be finite and > 0");
    if (d->n_tbins < 0 || d->n_tbins > TI_VLOSS_MAX_TBINS) return fail(TI_E_ARG, "n_tbins must be in 0.." + std::to_string(TI_VLOSS_MAX_TBINS));
    if (B < 1) return fail(TI_E_ARG, "B < 1");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (!two && z) return fail(TI_E_ARG, "the one-sided loss takes its noise as x0: z must be NULL");
    if (d->t_dist == TI_TDIST_GIVEN && !t) return fail(TI_E_ARG, "t_dist GIVEN needs t");
    if (d->t_dist != TI_TDIST_GIVEN && t) return fail(TI_E_ARG, "t is drawn by this t_dist: t must be NULL");
    if (t && mem == TI_MEM_HOST) {
        const bool open = two && d->gamma == TI_GAMMA_BROWNIAN;             // gamma' is infinite at both ends
        for (int64_t b = 0; b < B; ++b) {
            if (!(t[b] >= 0.0f && t[b] <= 1.0f)) return fail(TI_E_ARG, "t[" + std::to_string(b) + "] is outside [0, 1]");
            if (open && (t[b] == 0.0f || t[b] == 1.0f)) return fail(TI_E_ARG, "t[" + std::to_string(b) + "] is 0 or 1, where the brownian gamma' is infinite");
        }
    }
    return TI_OK;
}

namespace {

// c0 / c1: cond / NULL of a painn handle, beta0 / beta1 of an adw handle.  interp_only: stage one alone (out_xt required).
int vloss_impl(ti_handle* h, int want_kind, const ti_vloss_desc* d, const float* x0, const float* x1, const float* c0, const float* c1,
               const float* t, const float* z, int64_t B, double* out_loss, double* out_mean, double* out_tbins, float* out_t, float* out_z,
               float* out_xt, float* out_b, int mem, bool interp_only)
{
    if (int rc = vloss_check(d, t, z, B, mem)) return rc;
    if (!x0 || !x1 || (interp_only ? !out_xt : !out_loss)) return fail(TI_E_ARG, "NULL buffer");
    if (!h || h->kind != want_kind) return fail(TI_E_ARG, want_kind == 0 ? "not a painn handle" : "not an adw handle");
    const bool painn = h->kind == 0, two = d->kind == TI_VLOSS_STANDARD;
    if (!interp_only && (painn ? (h->ncond > 0 && !c0) : (!c0 || !c1))) return fail(TI_E_ARG, "NULL buffer");
    if (painn && !h->natoms.empty()) return fail(TI_E_UNSUPPORTED, "the velocity loss takes one species per call: clear ti_painn_set_molecules first");
    if (!painn && d->center != TI_CENTER_NONE) return fail(TI_E_UNSUPPORTED, "an adw handle takes TI_CENTER_NONE only");
    if (painn && !interp_only && h->tap >= 0) return fail(TI_E_ARG, MSG_TAP_ENTRIES);
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const bool host = mem == TI_MEM_HOST;
        const int A = painn ? h->d.n_atoms : 1, m = painn ? 3 * A : h->a_dim, nc = m / A, halves = two ? 2 : 1;
        const size_t n = (size_t)B * m, rows = (size_t)B * A;
        auto in = [&](const float* p, DevBuf<float>& buf, size_t cnt) -> const float* {
            if (!p || !host) return p;
            grow(buf, cnt);
            HIP_CHECK(hipMemcpyAsync(buf.p, p, cnt * sizeof(float), hipMemcpyHostToDevice, st));
            return buf.p;
        };
        // ---- the layout of the states.  One evaluation of the drift takes [xt+; xt-] as it stands in vl_xt.  A layout that packs G > 1
        // molecules into a row group makes a molecule's per-atom sums follow its slot in the group, so there the batch is laid out with
        // molecule b of either half at slot (traj_offset + b) mod G: `pad` copies of the call's first molecule in front of the plus half,
        // `pad2` between the halves, their results dropped.  The interpolate kernels write the halves where they belong (VlossParams::half)
        // and the drift reads and writes in place: no pass over the states is added.  With an edge mask in force (for B molecules) the
        // halves are evaluated one after the other as two batches of B, unaligned: the mask's rows are the call's.
        const bool eval = !interp_only, masked = eval && painn && h->emask_B > 0;
        long long pad = 0, pad2 = 0, nbp = masked ? B : (long long)halves * B;
        if (eval && painn) {
            select_template(h, nbp);
            for (int pass = 0; pass < 8 && !masked; ++pass) {           // to a fixed point: the padded count may choose a layout with another G
                const long long G = h->G;
                pad = G > 1 ? ((d->traj_offset % G) + G) % G : 0;
                pad2 = G > 1 && two ? (G - B % G) % G : 0;
                nbp = pad + B + (two ? pad2 + B : 0);
                select_template(h, nbp);
                if (h->G == G) break;
                if (pass == 7) { pad = pad2 = 0; nbp = (long long)halves * B; select_template(h, nbp); }      // no fixed point: unaligned
            }
        }
        const size_t half = (size_t)(B + pad2) * m, lead = (size_t)pad * m;
        // every buffer of the call at its final size first: grow() does not keep contents
        grow(h->vl_red, (size_t)RED_TBINS + 2 * TI_VLOSS_MAX_TBINS);
        grow(h->vl_part, std::max<size_t>((size_t)vloss_tiles((long long)rows) * nc, (size_t)vloss_tiles(B)));
        grow(h->vl_xt, lead + half + n);
        if (two) grow(h->vl_z, n);
        if (d->center != TI_CENTER_NONE) grow(h->vl_raw, halves * n);
        const float *x0d = in(x0, h->vl_x0, n), *x1d = in(x1, h->vl_x1, n), *zin = in(z, h->vl_zin, n);
        const float* td = nullptr;
        if (d->t_dist == TI_TDIST_GIVEN) td = in(t, h->vl_t, (size_t)B);
        else {
            grow(h->vl_t, (size_t)B);
            HIP_CHECK(launch_vloss_draw_t(h->vl_t.p, d->t_dist, d->seed, d->traj_offset, d->draw, B, st));
            td = h->vl_t.p;
        }
        // ---- interpolate
        VlossParams p{};
        p.kind = d->kind; p.gamma = d->gamma; p.center = d->center; p.a = d->a;
        p.B = B; p.m = m; p.A = A;
        p.x0 = x0d; p.x1 = x1d; p.t = td; p.z_in = zin;
        p.seed = d->seed; p.traj0 = d->traj_offset; p.draw = d->draw;
        p.z = two ? h->vl_z.p : nullptr; p.raw = h->vl_raw.p; p.colsum = h->vl_red.p + RED_COLSUM;
        p.xt = h->vl_xt.p + lead; p.half = (long long)half;
        HIP_CHECK(launch_vloss_interp(p, st));
        if (d->center == TI_CENTER_BATCH)
            for (int hf = 0; hf < halves; ++hf)
                HIP_CHECK(launch_vloss_colsum(h->vl_red.p + RED_COLSUM + hf * nc, h->vl_part.p, h->vl_raw.p + (size_t)hf * n, (long long)rows, nc, st));
        if (d->center != TI_CENTER_NONE) HIP_CHECK(launch_vloss_center(p, st));
        const hipMemcpyKind out_kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        auto copy_out = [&](void* dst, const void* src, size_t bytes) { if (dst) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, out_kind, st)); };
        auto copy_halves = [&](float* dst, const float* src) {         // [2][B][m] for the caller from the two halves as they lie
            for (int hf = 0; dst && hf < halves; ++hf) copy_out(dst + (size_t)hf * n, src + (size_t)hf * half, n * sizeof(float));
        };
        auto copy_states = [&]() {
            if (out_t && out_t != td) copy_out(out_t, td, (size_t)B * sizeof(float));
            if (two) copy_out(out_z, h->vl_z.p, n * sizeof(float));
            copy_halves(out_xt, p.xt);
        };
        if (interp_only) {
            copy_states();
            HIP_CHECK(hipStreamSynchronize(st));
            return TI_OK;
        }
        // ---- drift: times and conditioning of the evaluated batch, segment by segment like the states
        auto d2d = [&](float* dst, const float* src, size_t cnt) {
            if (cnt) HIP_CHECK(hipMemcpyAsync(dst, src, cnt * sizeof(float), hipMemcpyDeviceToDevice, st));
        };
        auto laid_out = [&](const float* src, DevBuf<float>& buf, size_t per) -> const float* {      // per floats per molecule
            if (!src || !per || nbp == B) return src;
            grow(buf, (size_t)nbp * per);
            float* q = buf.p;
            for (int hf = 0; hf < halves; ++hf) {
                for (long long k = 0; k < (hf ? pad2 : pad); ++k, q += per) d2d(q, src, per);
                d2d(q, src, (size_t)B * per); q += (size_t)B * per;
            }
            return buf.p;
        };
        const size_t ncnd = painn ? rows * h->ncond : (size_t)B;
        const float *c0d = in(c0, h->vl_c0, ncnd), *c1d = painn ? nullptr : in(c1, h->vl_c1, ncnd);
        const float *te = laid_out(td, h->vl_t2, 1), *c0e = laid_out(c0d, h->vl_c02, ncnd / (size_t)B), *c1e = laid_out(c1d, h->vl_c12, 1);
        for (long long k = 0; k < pad; ++k) d2d(h->vl_xt.p + (size_t)k * m, p.xt, (size_t)m);                  // the pad molecules: copies of the first
        for (long long k = 0; k < pad2; ++k) d2d(p.xt + n + (size_t)k * m, p.xt, (size_t)m);
        grow(h->vl_b, lead + half + n);
        grow(h->vl_loss, (size_t)B);
        if (painn) {
            ensure_painn_ws(h, nbp);
            phi0_begin_call(h, c0e, nbp, false);          // per-molecule times: no table path, the call's class state is reset
            struct Phi0End { ti_handle* h; ~Phi0End() { phi0_end_call(h); } } phi0_end{h};
            painn_drift_dev(h, h->vl_xt.p, 0.f, c0e, nbp, h->vl_b.p, nullptr, te);
            if (masked && two) painn_drift_dev(h, h->vl_xt.p + n, 0.f, c0e, nbp, h->vl_b.p + n, nullptr, te);
        } else {
            ensure_adw_ws(h, nbp);
            adw_drift_tv_dev(h, h->vl_xt.p, te, c0e, c1e, nbp, h->vl_b.p, nullptr);
        }
        // ---- reduce
        p.b = h->vl_b.p + lead; p.loss = h->vl_loss.p;
        HIP_CHECK(launch_vloss_reduce(p, st));
        HIP_CHECK(launch_vloss_first_bad(h->vl_red.p + RED_BAD, h->vl_loss.p, B, st));
        HIP_CHECK(launch_vloss_colsum(h->vl_red.p + RED_MEAN, h->vl_part.p, h->vl_loss.p, B, 1, st));
        if (d->n_tbins > 0) HIP_CHECK(launch_vloss_tbins(h->vl_red.p + RED_TBINS, h->vl_loss.p, td, B, d->n_tbins, st));
        std::vector<double> red(2 + 2 * (size_t)d->n_tbins);
        HIP_CHECK(hipMemcpyAsync(red.data(), h->vl_red.p + RED_MEAN, red.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (red[1] < (double)B) return fail(TI_E_NAN, "non-finite loss in molecule " + std::to_string((long long)red[1]));
        if (out_mean) *out_mean = red[0] / (double)rows;
        if (out_tbins) std::copy(red.begin() + 2, red.end(), out_tbins);
        copy_states();
        copy_out(out_loss, h->vl_loss.p, (size_t)B * sizeof(double));
        copy_halves(out_b, p.b);
        HIP_CHECK(hipStreamSynchronize(st));
        return TI_OK;
    });
}

}  // namespace

extern "C" {

int ti_painn_vloss(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* cond, const float* t,
                   const float* z, int64_t B, double* out_loss, double* out_mean, double* out_tbins, float* out_t, float* out_z,
                   float* out_xt, float* out_b, int mem)
{
    return vloss_impl(h, 0, desc, x0, x1, cond, nullptr, t, z, B, out_loss, out_mean, out_tbins, out_t, out_z, out_xt, out_b, mem, false);
}

int ti_adw_vloss(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* beta0, const float* beta1,
                 const float* t, const float* z, int64_t B, double* out_loss, double* out_mean, double* out_tbins, float* out_t,
                 float* out_z, float* out_xt, float* out_b, int mem)
{
    return vloss_impl(h, 1, desc, x0, x1, beta0, beta1, t, z, B, out_loss, out_mean, out_tbins, out_t, out_z, out_xt, out_b, mem, false);
}

int ti_painn_vloss_interp(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* t, const float* z,
                          int64_t B, float* out_t, float* out_z, float* out_xt, int mem)
{
    return vloss_impl(h, 0, desc, x0, x1, nullptr, nullptr, t, z, B, nullptr, nullptr, nullptr, out_t, out_z, out_xt, nullptr, mem, true);
}

int ti_adw_vloss_interp(ti_handle* h, const ti_vloss_desc* desc, const float* x0, const float* x1, const float* t, const float* z,
                        int64_t B, float* out_t, float* out_z, float* out_xt, int mem)
{
    return vloss_impl(h, 1, desc, x0, x1, nullptr, nullptr, t, z, B, nullptr, nullptr, nullptr, out_t, out_z, out_xt, nullptr, mem, true);
}

}  // extern "C"
