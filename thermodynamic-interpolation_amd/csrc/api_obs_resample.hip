// api_obs_resample.hip -- C ABI of the estimators over resamples (include/ti_hip.h ti_obs_bootstrap, ti_obs_rff_gram,
// ti_obs_rff_gram_wide): checks, staging, the draws and the cut into launches.  Kernels: obs_boot_kernels.hip, obs_gram_kernels.hip.
#include "ti_handle.hpp"

// The bad-index flag of a call that may read caller-given index rows: cleared before the first launch that draws; its download is
// enqueued with the results, and after the caller's wait bad_idx_refusal turns it into the refusal for a population of n_pop.
static void bad_idx_clear(ti_handle* h)
{
    grow(h->boot_flag, 1);
    HIP_CHECK(hipMemsetAsync(h->boot_flag.p, 0, sizeof(int), h->stream));
}

static void bad_idx_fetch(ti_handle* h, int* flag) { HIP_CHECK(hipMemcpyAsync(flag, h->boot_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream)); }

static int bad_idx_refusal(int flag, long long n_pop) { return flag ? fail(TI_E_ARG, "idx entry outside 0.." + std::to_string(n_pop - 1)) : TI_OK; }

// numpy's default percentile of the sorted s at fraction p: linear between the neighbours of position (n - 1) p (numpy's _lerp)
static double percentile_sorted(const std::vector<double>& s, double p)
{
    const double pos = (double)(s.size() - 1) * p, fl = std::floor(pos), t = pos - fl;
    const size_t i = (size_t)fl;
    if (i + 1 >= s.size()) return s.back();
    const double a = s[i], b = s[i + 1];
    return t >= 0.5 ? b - (b - a) * (1.0 - t) : a + (b - a) * t;
}

// ti_obs_rff_gram (max_p = 128) and ti_obs_rff_gram_wide (max_p = TI_GRAM_WIDE_MAX_P): one body, so that the checks, the staging,
// the draws and the cut into launches are the same statement; more than 8 column tiles take the blocked pass
static int rff_gram_call(ti_handle* h, const float* values, int64_t stride, int64_t n, const double* omega, const float* logw,
                         const ti_gram_desc* g, const int32_t* idx, int64_t n_draw, double* out, int mem, int max_p)
{
    // the checks that need no device come first, so they can be exercised with a NULL handle; that one is refused last
    if (!values || !omega || !g || !out) return fail(TI_E_ARG, "NULL buffer");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n < 1 || n > (int64_t)INT32_MAX) return fail(TI_E_ARG, "n must be in 1..2^31-1");
    if (g->d < 1 || g->d > 16) return fail(TI_E_ARG, "d must be in 1..16");
    if (g->p < 1 || g->p > max_p) return fail(TI_E_ARG, "p must be in 1.." + std::to_string(max_p));
    if (stride < g->d) return fail(TI_E_ARG, "stride < d");
    for (int i = 0; i < g->d * g->p; ++i)
        if (!std::isfinite(omega[i])) return fail(TI_E_ARG, "non-finite omega at entry " + std::to_string(i));
    if (g->n_boot < 0 || g->n_boot > TI_BOOT_MAX_RESAMPLES) return fail(TI_E_ARG, "n_boot must be in 0..2^20");
    if (n_draw < 0 || n_draw > (int64_t)INT32_MAX) return fail(TI_E_ARG, "n_draw must be in 0..2^31-1");
    if (idx && n_draw < 1) return fail(TI_E_ARG, "idx needs n_draw >= 1");
    if (!h) return fail(TI_E_ARG, "NULL handle");
    const int d = g->d, p = g->p, P = gram_pad(p), T = P / 16, NT = T * (T + 1) / 2;
    if (n * P > ((int64_t)1 << 27)) return fail(TI_E_ALLOC, "the feature table would exceed 2 GiB (n * P > 2^27, P = p rounded up to 16)");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const long long nb = g->n_boot, nd = n_draw > 0 ? n_draw : n;
        Staged sg(h, mem);
        long long sd = stride;
        const float* xd = sg.in_cols(values, sd, n, d, h->gram_x);          // the d columns only
        const float* ld = logw ? sg.in(logw, h->obs_logw, (size_t)n) : nullptr;
        const int32_t* id = idx && nb > 0 ? sg.in(idx, h->boot_idx, (size_t)nb * (size_t)n_draw) : nullptr;
        obs_scratch(h);
        if (ld) {
            double norm[2];
            if (int rc = logw_shift_dev(h, ld, n, norm)) return rc;
            grow(h->gram_w, (size_t)n);
        }
        h->gram_omega.upload(std::vector<double>(omega, omega + (size_t)d * p));
        grow(h->gram_z, (size_t)n * 2 * P);
        HIP_CHECK(launch_obs_gram_features(h->gram_z.p, h->gram_w.p, xd, sd, n, d, p, h->gram_omega.p, ld, h->obs_red.p, st));
        // rows per launch: the partial tiles of a launch stay within 256 MiB
        const size_t pp = (size_t)p * p * 2, part_doubles = (size_t)NT * 512, max_parts = std::max<size_t>(((size_t)256 << 20) / (part_doubles * 8), 1);
        grow(h->gram_out, (size_t)(1 + nb) * pp);
        bad_idx_clear(h);
        GramParams gp{};
        gp.z = h->gram_z.p; gp.w = ld ? h->gram_w.p : nullptr; gp.T = T;
        gp.draw.n_pop = n; gp.draw.seed = g->seed; gp.draw.flag = h->boot_flag.p;
        auto run = [&](long long rows, long long draws, double* dst) {       // gp.draw.{source, idx, first} set by the caller, rows within the cap
            gp.draw.n_draw = draws;
            gp.nseg = (draws + GRAM_SEG - 1) / GRAM_SEG;
            grow(h->gram_part, (size_t)rows * (size_t)gp.nseg * part_doubles);
            gp.part = h->gram_part.p;
            HIP_CHECK(T > 8 ? launch_obs_gram_wide(gp, rows, st) : launch_obs_gram(gp, rows, st));
            HIP_CHECK(launch_obs_gram_reduce(dst, gp.part, rows, gp.nseg, p, st));
        };
        gp.draw.source = BOOT_SRC_IDENTITY;
        run(1, n, h->gram_out.p);
        const long long nseg = (nd + GRAM_SEG - 1) / GRAM_SEG, chunk = std::max<long long>((long long)max_parts / nseg, 1);
        for (long long r0 = 0; r0 < nb; r0 += chunk) {
            gp.draw.source = id ? BOOT_SRC_INDEX : BOOT_SRC_PHILOX;
            gp.draw.idx = id ? id + r0 * nd : nullptr;
            gp.draw.first = (long long)((uint64_t)g->first + (uint64_t)r0);
            run(std::min(chunk, nb - r0), nd, h->gram_out.p + (size_t)(1 + r0) * pp);
        }
        int flag = 0;
        bad_idx_fetch(h, &flag);
        HIP_CHECK(hipStreamSynchronize(st));
        if (int rc = bad_idx_refusal(flag, n)) return rc;
        HIP_CHECK(hipMemcpyAsync(out, h->gram_out.p, (size_t)(1 + nb) * pp * sizeof(double), out_kind(mem), st));
        HIP_CHECK(hipStreamSynchronize(st));
        return TI_OK;
    });
}

extern "C" {

int ti_obs_bootstrap(ti_handle* h, const float* logw, int64_t n, const ti_boot_desc* d, const int32_t* idx, int64_t n_draw, double* out,
                     double* out_boot, int mem)
{
    // the checks that need no device come first, so they can be exercised with a NULL handle; that one is refused last
    if (!logw || !d || !out) return fail(TI_E_ARG, "NULL buffer");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n < 1 || n > (int64_t)INT32_MAX) return fail(TI_E_ARG, "n must be in 1..2^31-1");
    if (d->estimator < TI_BOOT_ESS || d->estimator > TI_BOOT_MEAN) return fail(TI_E_ARG, "unknown estimator");
    if (d->filter < TI_BOOT_FILTER_NONE || d->filter > TI_BOOT_FILTER_RESAMPLE) return fail(TI_E_ARG, "unknown filter");
    if (d->filter != TI_BOOT_FILTER_NONE && !(std::isfinite(d->k) && d->k > 0.0)) return fail(TI_E_ARG, "k must be finite and > 0");
    if (!(d->level > 0.0 && d->level < 1.0)) return fail(TI_E_ARG, "level must be in (0, 1)");
    if (d->n_boot < 0 || d->n_boot > TI_BOOT_MAX_RESAMPLES) return fail(TI_E_ARG, "n_boot must be in 0..2^20");
    if (n_draw < 0 || n_draw > (int64_t)INT32_MAX) return fail(TI_E_ARG, "n_draw must be in 0..2^31-1");
    if (idx && n_draw < 1) return fail(TI_E_ARG, "idx needs n_draw >= 1");
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const long long nb = d->n_boot;
        const bool mean = d->estimator == TI_BOOT_MEAN, filtered = d->filter != TI_BOOT_FILTER_NONE;
        Staged sg(h, mem);
        const float* ld = sg.in(logw, h->obs_logw, (size_t)n);
        const int32_t* id = idx && nb > 0 ? sg.in(idx, h->boot_idx, (size_t)nb * (size_t)n_draw) : nullptr;
        double norm[2];
        if (int rc = logw_shift_dev(h, ld, n, norm)) return rc;
        // the point estimate: the identity row, filtered once; ONCE: its survivors become the population
        grow(h->boot_pt, 5);
        grow(h->boot_est, (size_t)std::max<long long>(nb, 1));
        bad_idx_clear(h);
        BootParams p{};
        p.v = ld; p.n_pop = n; p.n_draw = n; p.source = BOOT_SRC_IDENTITY;
        p.estimator = d->estimator; p.filter = filtered; p.k = d->k; p.m = norm[0];
        p.seed = d->seed; p.first = d->first;
        p.est = h->boot_pt.p; p.kept = h->boot_pt.p + 1; p.bounds = h->boot_pt.p + 2; p.flag = h->boot_flag.p;
        HIP_CHECK(launch_obs_boot(p, 1, st));
        long long n_pop = n;
        if (d->filter == TI_BOOT_FILTER_ONCE) {
            grow(h->boot_pop, (size_t)n);
            HIP_CHECK(launch_obs_boot_compact(h->boot_pop.p, h->boot_pt.p + 4, ld, n, mean, norm[0], h->boot_pt.p + 2, st));
        }
        double pt[5] = {0, 0, 0, 0, 0};
        HIP_CHECK(hipMemcpyAsync(pt, h->boot_pt.p, sizeof(pt), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (d->filter == TI_BOOT_FILTER_ONCE) { n_pop = (long long)pt[4]; p.v = h->boot_pop.p; }
        // the resamples
        const long long nd = n_draw > 0 ? n_draw : n_pop;
        std::vector<double> est((size_t)nb, std::nan(""));
        if (id && n_pop == 0) return fail(TI_E_ARG, "idx entry outside the population (the filter kept nothing)");
        if (nb > 0 && n_pop > 0) {
            p.n_pop = n_pop; p.n_draw = nd; p.source = id ? BOOT_SRC_INDEX : BOOT_SRC_PHILOX; p.idx = id;
            p.filter = d->filter == TI_BOOT_FILTER_RESAMPLE;
            p.est = h->boot_est.p; p.kept = nullptr; p.bounds = nullptr;
            HIP_CHECK(launch_obs_boot(p, nb, st));
            int flag = 0;
            bad_idx_fetch(h, &flag);
            HIP_CHECK(hipMemcpyAsync(est.data(), h->boot_est.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (int rc = bad_idx_refusal(flag, n_pop)) return rc;
        }
        double lower = std::nan(""), upper = std::nan("");
        if (nb > 0 && std::none_of(est.begin(), est.end(), [](double e) { return std::isnan(e); })) {
            std::vector<double> s(est);
            std::sort(s.begin(), s.end());
            lower = percentile_sorted(s, (1.0 - d->level) / 2.0);
            upper = percentile_sorted(s, (1.0 + d->level) / 2.0);
        }
        out[0] = pt[0]; out[1] = lower; out[2] = upper; out[3] = pt[1];
        if (out_boot && nb > 0) {
            if (mem == TI_MEM_HOST) std::copy(est.begin(), est.end(), out_boot);
            else {                                         // nothing ran on an empty population: the NaN row comes from the host
                if (n_pop > 0) HIP_CHECK(hipMemcpyAsync(out_boot, h->boot_est.p, (size_t)nb * sizeof(double), out_kind(mem), st));
                else HIP_CHECK(hipMemcpyAsync(out_boot, est.data(), (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
                HIP_CHECK(hipStreamSynchronize(st));
            }
        }
        return TI_OK;
    });
}

int ti_obs_rff_gram(ti_handle* h, const float* values, int64_t stride, int64_t n, const double* omega, const float* logw,
                    const ti_gram_desc* g, const int32_t* idx, int64_t n_draw, double* out, int mem)
{
    return rff_gram_call(h, values, stride, n, omega, logw, g, idx, n_draw, out, mem, 128);
}

int ti_obs_rff_gram_wide(ti_handle* h, const float* values, int64_t stride, int64_t n, const double* omega, const float* logw,
                         const ti_gram_desc* g, const int32_t* idx, int64_t n_draw, double* out, int mem)
{
    return rff_gram_call(h, values, stride, n, omega, logw, g, idx, n_draw, out, mem, TI_GRAM_WIDE_MAX_P);
}

}  // extern "C"
