// api_obs.hip -- observables (ti_obs_*) that turn states or log-weights into per-sample numbers and histograms: collective variables
// of a state and the observer a rollout writes CV rows through, importance weights, weighted histograms of one column or of all, the
// TI log-weights and the Boltzmann-generator log-weights.  The reductions the other observables units share are defined here.
#include "ti_handle.hpp"

// Validates desc [K][5] against the handle (before any device work) and uploads it with ref / select into set `which`.
static int obs_upload(ti_handle* h, int which, const int32_t* desc, int K, const float* ref, const int32_t* select)
{
    if (h->kind >= 2) return fail(TI_E_ARG, "a trainer handle has no trajectories to observe");
    if (K < 1) return fail(TI_E_ARG, "K must be >= 1");
    const int A = h->kind == 0 ? h->d.n_atoms : 1, dim = h->a_dim;
    bool rmsd = false;
    for (int k = 0; k < K; ++k) {
        const int32_t* d = desc + 5 * k;
        const int kind = d[0];
        if (kind < TI_OBS_RMSD || kind > TI_OBS_COORD) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": unknown kind " + std::to_string(kind));
        if (h->kind == 1) {
            if (kind != TI_OBS_COORD) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": an adw handle takes COORD(c) only");
            if (d[1] < 0 || d[1] >= dim) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": component outside 0.." + std::to_string(dim - 1));
            continue;
        }
        if (kind == TI_OBS_COORD) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": COORD(c) is for adw handles");
        if (kind == TI_OBS_RMSD) { rmsd = true; continue; }
        const int na = kind == TI_OBS_DIST ? 2 : kind == TI_OBS_ANGLE ? 3 : 4;
        for (int j = 0; j < na; ++j)
            if (d[1 + j] < 0 || d[1 + j] >= A) return fail(TI_E_ARG, "descriptor " + std::to_string(k) + ": atom index outside 0.." + std::to_string(A - 1));
    }
    if (rmsd && !ref) return fail(TI_E_ARG, "an RMSD descriptor needs ref");
    set_device(h);
    ti_handle::ObsSet& o = h->obs[which];
    o.K = 0;
    o.desc.upload(std::vector<int32_t>(desc, desc + 5 * (size_t)K));
    o.has_ref = rmsd; o.has_sel = rmsd && select;
    if (o.has_ref) o.ref.upload(std::vector<float>(ref, ref + 3 * (size_t)A));
    if (o.has_sel) o.sel.upload(std::vector<int32_t>(select, select + A));
    o.K = K;
    return TI_OK;
}

namespace ti {

// cv_dev [B][K] = the CVs of set `which` on x_dev [B][m]; enqueued on the handle's stream
void obs_cv_dev(ti_handle* h, int which, const float* x_dev, long long B, float* cv_dev)
{
    const ti_handle::ObsSet& o = h->obs[which];
    if (h->kind == 0 && h->emask_B > 0 && B != h->emask_B)
        throw std::invalid_argument("the molecule state in force is for " + std::to_string(h->emask_B) + " molecules, the call has " + std::to_string(B));
    ObsCvParams p{};
    p.x = x_dev; p.B = B; p.A = h->kind == 0 ? h->d.n_atoms : 1; p.m = obs_floats_per_traj(h); p.K = o.K;
    p.desc = o.desc.p; p.ref = o.has_ref ? o.ref.p : nullptr; p.sel = o.has_sel ? o.sel.p : nullptr;
    p.n_atoms = h->kind == 0 && h->ragged ? h->natoms_dev.p : nullptr;
    p.cv = cv_dev;
    HIP_CHECK(launch_obs_cv(p, h->stream));
}

// The fp64 scratch of the reductions: h->obs_red holds 4 + words doubles, h->obs_part `words` per block.  grow never shrinks and does
// not keep contents.  So a call that needs more than the default per block (ti_obs_hist_cols) asks for it before anything is written
// into the scratch, and the later calls with the default, those inside the helpers below among them, leave the buffers where they are.
void obs_scratch(ti_handle* h, size_t words)
{
    grow(h->obs_red, 4 + words);
    grow(h->obs_part, (size_t)OBS_MAX_BLOCKS * words);
}

// The shift of the log-weights logw_dev [n] and their refusal: (max, first bad index) into h->obs_red[0..1] and `out`, one wait;
// TI_E_NAN on a non-finite entry
int logw_shift_dev(ti_handle* h, const float* logw_dev, long long n, double out[2])
{
    hipStream_t st = h->stream;
    obs_scratch(h);
    HIP_CHECK(launch_obs_logw_max(h->obs_red.p, h->obs_part.p, logw_dev, n, st));
    HIP_CHECK(hipMemcpyAsync(out, h->obs_red.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (out[1] < (double)n) return fail(TI_E_NAN, "non-finite logw at index " + std::to_string((long long)out[1]));
    return TI_OK;
}

}  // namespace ti

// (max, first bad index, sum w, sum w^2) of logw_dev into h->obs_red[0..3] and `norm`; TI_E_NAN on a non-finite entry
static int obs_norm_dev(ti_handle* h, const float* logw_dev, long long B, double norm[4])
{
    hipStream_t st = h->stream;
    if (int rc = logw_shift_dev(h, logw_dev, B, norm)) return rc;
    HIP_CHECK(launch_obs_logw_sums(h->obs_red.p + 2, h->obs_part.p, logw_dev, h->obs_red.p, B, st));
    HIP_CHECK(hipMemcpyAsync(norm + 2, h->obs_red.p + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    // the kernels that follow read (max, sum w) as one pair
    HIP_CHECK(hipMemcpyAsync(h->obs_red.p + 1, h->obs_red.p + 2, sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return TI_OK;
}

extern "C" {

int ti_obs_cv(ti_handle* h, const int32_t* desc, int32_t K, const float* ref, const int32_t* select, const float* x, int64_t B,
              float* out_cv, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (!desc) return fail(TI_E_ARG, "desc is NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (B < 0 || (B > 0 && (!x || !out_cv))) return fail(TI_E_ARG, "NULL buffer");
    return guarded([&]() -> int {
        if (int rc = obs_upload(h, 0, desc, K, ref, select)) return rc;
        if (B == 0) return TI_OK;
        Staged sg(h, mem);
        const float* xd = sg.in(x, h->obs_x, (size_t)B * obs_floats_per_traj(h));
        float* od = sg.out(out_cv, h->obs_cv, (size_t)B * K);
        obs_cv_dev(h, 0, xd, B, od);
        sg.finish();
        return TI_OK;
    });
}

int ti_obs_set_observer(ti_handle* h, const int32_t* desc, int32_t K, const float* ref, const int32_t* select, int32_t every,
                        float* out_cv, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (!desc) { h->obs[1].K = 0; h->obs_out = nullptr; return TI_OK; }
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (every < 0) return fail(TI_E_ARG, "every must be >= 0");
    if (!out_cv) return fail(TI_E_ARG, "out_cv is NULL");
    return guarded([&]() -> int {
        if (int rc = obs_upload(h, 1, desc, K, ref, select)) return rc;
        h->obs_every = every; h->obs_mem = mem; h->obs_out = out_cv;
        return TI_OK;
    });
}

int ti_obs_weights(ti_handle* h, const float* logw, int64_t B, float* out_w, double* out_ess, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (B < 1) return fail(TI_E_ARG, "B < 1");
    if (!logw || !out_ess) return fail(TI_E_ARG, "NULL buffer");
    return guarded([&]() -> int {
        set_device(h);
        Staged sg(h, mem);
        const float* ld = sg.in(logw, h->obs_logw, (size_t)B);
        float* wd = out_w ? sg.out(out_w, h->obs_w, (size_t)B) : nullptr;
        double norm[4];
        if (int rc = obs_norm_dev(h, ld, B, norm)) return rc;
        *out_ess = norm[2] * norm[2] / norm[3];
        if (out_w) {
            HIP_CHECK(launch_obs_weights(wd, ld, h->obs_red.p, B, h->stream));
            sg.finish();
        }
        return TI_OK;
    });
}

int ti_obs_hist(ti_handle* h, const float* values, int64_t stride, const float* logw, int64_t B, int32_t n_bins, double lo, double hi,
                double* out_hist, double* out_tails, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n_bins < 1 || n_bins > 256) return fail(TI_E_ARG, "n_bins must be in 1..256");
    if (!(hi > lo) || !std::isfinite(lo) || !std::isfinite(hi)) return fail(TI_E_ARG, "the range needs finite lo < hi");
    if (B < 1 || stride < 1) return fail(TI_E_ARG, "B < 1 or stride < 1");
    if (!values || !out_hist || !out_tails) return fail(TI_E_ARG, "NULL buffer");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        Staged sg(h, mem);
        long long sd = stride;
        const float* vd = sg.in_cols(values, sd, B, 1, h->obs_val);         // the column only: B floats, not B * stride
        const float* ld = sg.in(logw, h->obs_logw, (size_t)B);
        double norm[4];
        if (ld) { if (int rc = obs_norm_dev(h, ld, B, norm)) return rc; }
        else obs_scratch(h);
        HIP_CHECK(launch_obs_whist(h->obs_red.p + 4, h->obs_part.p, vd, sd, ld, h->obs_red.p, B, n_bins, lo, hi, st));
        std::vector<double> out((size_t)n_bins + 3);
        HIP_CHECK(hipMemcpyAsync(out.data(), h->obs_red.p + 4, out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::copy(out.begin(), out.begin() + n_bins, out_hist);
        std::copy(out.begin() + n_bins, out.end(), out_tails);
        return TI_OK;
    });
}

int ti_obs_hist_cols(ti_handle* h, const float* values, int32_t K, const float* logw, const uint8_t* keep, int64_t B, int32_t n_bins,
                     const double* lo, const double* hi, double* out_hist, double* out_tails, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n_bins < 1 || n_bins > 256) return fail(TI_E_ARG, "n_bins must be in 1..256");
    if (K < 1 || K > HIST_COLS_MAX) return fail(TI_E_ARG, "K must be in 1.." + std::to_string(HIST_COLS_MAX));
    if (B < 1) return fail(TI_E_ARG, "B < 1");
    if (!values || !lo || !hi || !out_hist || !out_tails) return fail(TI_E_ARG, "NULL buffer");
    for (int c = 0; c < K; ++c)
        if (!(hi[c] > lo[c]) || !std::isfinite(lo[c]) || !std::isfinite(hi[c])) return fail(TI_E_ARG, "column " + std::to_string(c) + ": the range needs finite lo < hi");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const size_t ncol = (size_t)n_bins + 3;
        Staged sg(h, mem);
        const float* vd = sg.in(values, h->obs_val, (size_t)B * K);
        const float* ld = logw ? sg.in(logw, h->obs_logw, (size_t)B) : nullptr;
        const uint8_t* kd = keep ? sg.in(keep, h->hc_keep, (size_t)B) : nullptr;
        std::vector<double> range(lo, lo + K);
        range.insert(range.end(), hi, hi + K);
        h->hc_range.upload(range);
        obs_scratch(h, std::max<size_t>((size_t)K * ncol, 259));           // K columns a block, ahead of the reductions (obs_scratch)
        double m = 0.0, tot = (double)B;
        if (kd) {                                          // the shift, the refusal and the normalising sum over the kept entries
            double r[3];
            HIP_CHECK(launch_obs_keep_max(h->obs_red.p, h->obs_part.p, ld, kd, B, st));
            HIP_CHECK(hipMemcpyAsync(r, h->obs_red.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (r[2] < 1.0) return fail(TI_E_ARG, "keep keeps no entry");
            if (r[1] < (double)B) return fail(TI_E_NAN, "non-finite logw at index " + std::to_string((long long)r[1]));
            tot = r[2];
            if (ld) {
                m = r[0];
                HIP_CHECK(launch_obs_keep_sum(h->obs_red.p, h->obs_part.p, ld, kd, m, B, st));
                HIP_CHECK(hipMemcpyAsync(&tot, h->obs_red.p, sizeof(double), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
            }
        } else if (ld) {                                   // the reductions of ti_obs_weights / ti_obs_hist
            double norm[4];
            if (int rc = obs_norm_dev(h, ld, B, norm)) return rc;
            m = norm[0]; tot = norm[2];
        }
        HIP_CHECK(launch_obs_whist_cols(h->obs_red.p + 4, h->obs_part.p, vd, K, ld, kd, m, tot, B, n_bins, h->hc_range.p, h->hc_range.p + K, st));
        std::vector<double> out((size_t)K * ncol);
        HIP_CHECK(hipMemcpyAsync(out.data(), h->obs_red.p + 4, out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int c = 0; c < K; ++c) {
            std::copy(out.begin() + c * ncol, out.begin() + c * ncol + n_bins, out_hist + (size_t)c * n_bins);
            std::copy(out.begin() + c * ncol + n_bins, out.begin() + (c + 1) * ncol, out_tails + (size_t)c * 3);
        }
        return TI_OK;
    });
}

int ti_obs_ti_logw(ti_handle* h, const double* u0, const double* u1, const float* neg_dlogp, int64_t B, float* out_logw, int mem)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (B < 1) return fail(TI_E_ARG, "B < 1");
    if (!u1 || !out_logw) return fail(TI_E_ARG, "NULL buffer");
    return guarded([&]() -> int {
        set_device(h);
        Staged sg(h, mem);
        const double* u0d = u0 ? sg.in(u0, h->ff_u0, (size_t)B) : nullptr;
        const double* u1d = sg.in(u1, h->ff_u1, (size_t)B);
        const float* nd = neg_dlogp ? sg.in(neg_dlogp, h->obs_val, (size_t)B) : nullptr;
        float* od = sg.out(out_logw, h->obs_logw, (size_t)B);
        HIP_CHECK(launch_obs_ti_logw(od, u0d, u1d, nd, B, h->stream));
        sg.finish();
        return TI_OK;
    });
}

int ti_obs_bg_logw(ti_handle* h, const float* z, int64_t B, int64_t m, const double* u1, const float* neg_dlogp_bg, const float* neg_dlogp_ti,
                   double* out_logpz, float* out_logw, int mem)
{
    // the checks that need no device come first, so they can be exercised with a NULL handle; that one is refused last
    if (!z) return fail(TI_E_ARG, "z is NULL");
    if (!out_logpz && !out_logw) return fail(TI_E_ARG, "out_logpz and out_logw are both NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (B < 1) return fail(TI_E_ARG, "B < 1");
    if (m < 1 || m > TI_BG_MAX_M) return fail(TI_E_ARG, "m must be in 1.." + std::to_string(TI_BG_MAX_M));
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        Staged sg(h, mem);
        BgParams p{};
        p.B = B; p.m = (int)m;
        p.z = sg.in(z, h->obs_x, (size_t)B * (size_t)m);
        p.u1 = u1 ? sg.in(u1, h->ff_u1, (size_t)B) : nullptr;
        p.nd_bg = neg_dlogp_bg ? sg.in(neg_dlogp_bg, h->obs_val, (size_t)B) : nullptr;
        p.nd_ti = neg_dlogp_ti ? sg.in(neg_dlogp_ti, h->bg_nt, (size_t)B) : nullptr;
        p.logpz = out_logpz ? sg.out(out_logpz, h->bg_logpz, (size_t)B) : nullptr;
        p.logw = out_logw ? sg.out(out_logw, h->obs_logw, (size_t)B) : nullptr;
        HIP_CHECK(launch_obs_bg_logw(p, h->stream));
        sg.finish();
        return TI_OK;
    });
}

int ti_obs_bg_ess(ti_handle* h, const double* logpz, int64_t B, const double* u1, const float* neg_dlogp_bg, const float* neg_dlogp_ti,
                  const uint8_t* keep, double* out_ess, int64_t* out_kept, int mem)
{
    if (!logpz || !out_ess) return fail(TI_E_ARG, "NULL buffer");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (B < 1) return fail(TI_E_ARG, "B < 1");
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        Staged sg(h, mem);
        BgEssParams p{};
        p.B = B;
        p.logpz = sg.in(logpz, h->bg_logpz, (size_t)B);
        p.u1 = u1 ? sg.in(u1, h->ff_u1, (size_t)B) : nullptr;
        p.nd_bg = neg_dlogp_bg ? sg.in(neg_dlogp_bg, h->obs_val, (size_t)B) : nullptr;
        p.nd_ti = neg_dlogp_ti ? sg.in(neg_dlogp_ti, h->bg_nt, (size_t)B) : nullptr;
        p.keep = keep ? sg.in(keep, h->hc_keep, (size_t)B) : nullptr;
        obs_scratch(h);
        p.out = h->obs_red.p;
        HIP_CHECK(launch_obs_bg_ess(p, h->stream));
        double r[3];
        HIP_CHECK(hipMemcpyAsync(r, h->obs_red.p, sizeof r, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (r[1] < 1.0) return fail(TI_E_ARG, "keep leaves no molecule");
        if (r[2] < (double)B) return fail(TI_E_NAN, "non-finite log-weight at index " + std::to_string((long long)r[2]));
        *out_ess = r[0];
        if (out_kept) *out_kept = (int64_t)r[1];
        return TI_OK;
    });
}

}  // extern "C"
