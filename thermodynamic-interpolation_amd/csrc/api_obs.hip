// api_obs.hip -- observables (ti_obs_*): collective variables of a state, importance weights, weighted histograms, force-field
// energies and the TI log-weights formed from them, the Boltzmann-generator log-weights, Z-matrix coordinates both ways, and the
// observer a rollout writes CV rows through.
#include "ti_handle.hpp"

namespace {

// Validates desc [K][5] against the handle (before any device work) and uploads it with ref / select into set `which`.
int obs_upload(ti_handle* h, int which, const int32_t* desc, int K, const float* ref, const int32_t* select)
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

}  // namespace

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

}  // namespace ti

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

// (max, first bad index, sum w, sum w^2) of logw_dev into h->obs_red[0..3] and `norm`; TI_E_NAN on a non-finite entry
static int obs_norm_dev(ti_handle* h, const float* logw_dev, long long B, double norm[4])
{
    hipStream_t st = h->stream;
    grow(h->obs_red, 4 + 259);
    grow(h->obs_part, (size_t)OBS_MAX_BLOCKS * 259);
    HIP_CHECK(launch_obs_logw_max(h->obs_red.p, h->obs_part.p, logw_dev, B, st));
    HIP_CHECK(hipMemcpyAsync(norm, h->obs_red.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (norm[1] < (double)B) return fail(TI_E_NAN, "non-finite logw at index " + std::to_string((long long)norm[1]));
    HIP_CHECK(launch_obs_logw_sums(h->obs_red.p + 2, h->obs_part.p, logw_dev, h->obs_red.p, B, st));
    HIP_CHECK(hipMemcpyAsync(norm + 2, h->obs_red.p + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    // the kernels that follow read (max, sum w) as one pair
    HIP_CHECK(hipMemcpyAsync(h->obs_red.p + 1, h->obs_red.p + 2, sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return TI_OK;
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

// numpy's default percentile of the sorted s at fraction p: linear between the neighbours of position (n - 1) p (numpy's _lerp)
static double percentile_sorted(const std::vector<double>& s, double p)
{
    const double pos = (double)(s.size() - 1) * p, fl = std::floor(pos), t = pos - fl;
    const size_t i = (size_t)fl;
    if (i + 1 >= s.size()) return s.back();
    const double a = s[i], b = s[i + 1];
    return t >= 0.5 ? b - (b - a) * (1.0 - t) : a + (b - a) * t;
}

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
        // the shift and the refusal of ti_obs_weights
        grow(h->obs_red, 4 + 259);
        grow(h->obs_part, (size_t)OBS_MAX_BLOCKS * 259);
        double norm[2];
        HIP_CHECK(launch_obs_logw_max(h->obs_red.p, h->obs_part.p, ld, n, st));
        HIP_CHECK(hipMemcpyAsync(norm, h->obs_red.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (norm[1] < (double)n) return fail(TI_E_NAN, "non-finite logw at index " + std::to_string((long long)norm[1]));
        // the point estimate: the identity row, filtered once; ONCE: its survivors become the population
        grow(h->boot_pt, 5);
        grow(h->boot_flag, 1);
        grow(h->boot_est, (size_t)std::max<long long>(nb, 1));
        HIP_CHECK(hipMemsetAsync(h->boot_flag.p, 0, sizeof(int), st));
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
            HIP_CHECK(hipMemcpyAsync(&flag, h->boot_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(est.data(), h->boot_est.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (flag) return fail(TI_E_ARG, "idx entry outside 0.." + std::to_string(n_pop - 1));
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
            else if (n_pop > 0) {
                HIP_CHECK(hipMemcpyAsync(out_boot, h->boot_est.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToDevice, st));
                HIP_CHECK(hipStreamSynchronize(st));
            } else {
                HIP_CHECK(hipMemcpyAsync(out_boot, est.data(), (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
                HIP_CHECK(hipStreamSynchronize(st));
            }
        }
        return TI_OK;
    });
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
        const float* xd = values;
        long long sd = stride;
        if (mem == TI_MEM_HOST) {                      // the d columns only
            std::vector<float> rows((size_t)n * d);
            for (int64_t i = 0; i < n; ++i) std::copy(values + i * stride, values + i * stride + d, rows.begin() + i * d);
            grow(h->gram_x, rows.size());
            HIP_CHECK(hipMemcpy(h->gram_x.p, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
            xd = h->gram_x.p; sd = d;
        }
        const float* ld = logw ? sg.in(logw, h->obs_logw, (size_t)n) : nullptr;
        const int32_t* id = idx && nb > 0 ? sg.in(idx, h->boot_idx, (size_t)nb * (size_t)n_draw) : nullptr;
        grow(h->obs_red, 4 + 259);
        grow(h->obs_part, (size_t)OBS_MAX_BLOCKS * 259);
        if (ld) {                                      // the shift and the refusal of ti_obs_weights
            double norm[2];
            HIP_CHECK(launch_obs_logw_max(h->obs_red.p, h->obs_part.p, ld, n, st));
            HIP_CHECK(hipMemcpyAsync(norm, h->obs_red.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (norm[1] < (double)n) return fail(TI_E_NAN, "non-finite logw at index " + std::to_string((long long)norm[1]));
            grow(h->gram_w, (size_t)n);
        }
        h->gram_omega.upload(std::vector<double>(omega, omega + (size_t)d * p));
        grow(h->gram_z, (size_t)n * 2 * P);
        HIP_CHECK(launch_obs_gram_features(h->gram_z.p, h->gram_w.p, xd, sd, n, d, p, h->gram_omega.p, ld, h->obs_red.p, st));
        // rows per launch: the partial tiles of a launch stay within 256 MiB
        const size_t pp = (size_t)p * p * 2, part_doubles = (size_t)NT * 512, max_parts = std::max<size_t>(((size_t)256 << 20) / (part_doubles * 8), 1);
        grow(h->gram_out, (size_t)(1 + nb) * pp);
        grow(h->boot_flag, 1);
        HIP_CHECK(hipMemsetAsync(h->boot_flag.p, 0, sizeof(int), st));
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
        HIP_CHECK(hipMemcpyAsync(&flag, h->boot_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (flag) return fail(TI_E_ARG, "idx entry outside 0.." + std::to_string(n - 1));
        HIP_CHECK(hipMemcpyAsync(out, h->gram_out.p, (size_t)(1 + nb) * pp * sizeof(double),
                                 mem == TI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
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

// the refusals ti_obs_eigh and ti_obs_gedmd_spectrum find in the status words of a solve over n_mat matrices (host copy)
static int eig_status_refusal(const std::vector<int32_t>& st, const char* what)
{
    for (size_t i = 0; i < st.size(); ++i) {
        if (st[i] < 0) return fail(TI_E_NAN, std::string("non-finite entry in ") + what + " " + std::to_string(i));
        if (st[i] > EIG_MAX_SWEEPS)
            return fail(TI_E_UNSUPPORTED, std::string(what) + " " + std::to_string(i) + " is still rotating after " + std::to_string(EIG_MAX_SWEEPS) + " sweeps");
    }
    return TI_OK;
}

static int eig_n_mat_refusal(int64_t n_mat)
{
    if (n_mat < 1 || n_mat > (int64_t)TI_BOOT_MAX_RESAMPLES + 1) return fail(TI_E_ARG, "n_mat must be in 1..2^20+1");
    return TI_OK;
}

int ti_obs_eigh(ti_handle* h, const double* a, int64_t n_mat, int32_t n, double* w, double* v, int32_t* sweeps, int mem)
{
    // the checks that need no device come first, so they can be exercised with a NULL handle; that one is refused last
    if (!a) return fail(TI_E_ARG, "a is NULL");
    if (!w) return fail(TI_E_ARG, "w is NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n < 1 || n > TI_EIGH_MAX_N) return fail(TI_E_ARG, "n must be in 1..64");
    if (int rc = eig_n_mat_refusal(n_mat)) return rc;
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const size_t nn = (size_t)n * n * 2, N = (size_t)n_mat;
        Staged sg(h, mem);
        const double* ad = sg.in(a, h->eig_a, N * nn);
        grow(h->eig_w, N * n);
        if (v) grow(h->eig_v, N * nn);
        grow(h->eig_st, N);
        HIP_CHECK(launch_obs_eigh(ad, (long long)nn, n, n, nullptr, h->eig_w.p, v ? h->eig_v.p : nullptr, n, h->eig_st.p, n_mat, st));
        std::vector<int32_t> status(N);
        HIP_CHECK(hipMemcpyAsync(status.data(), h->eig_st.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (int rc = eig_status_refusal(status, "matrix")) return rc;
        const hipMemcpyKind kind = mem == TI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        HIP_CHECK(hipMemcpyAsync(w, h->eig_w.p, N * n * sizeof(double), kind, st));
        if (v) HIP_CHECK(hipMemcpyAsync(v, h->eig_v.p, N * nn * sizeof(double), kind, st));
        if (sweeps && mem == TI_MEM_DEVICE) HIP_CHECK(hipMemcpyAsync(sweeps, h->eig_st.p, N * sizeof(int32_t), kind, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (sweeps && mem == TI_MEM_HOST) std::copy(status.begin(), status.end(), sweeps);
        return TI_OK;
    });
}

int ti_obs_gedmd_spectrum(ti_handle* h, const double* gram, int64_t n_mat, const double* omega, const ti_gedmd_desc* g, double* ev, double* vec,
                          int32_t* rank, int mem)
{
    // the checks that need no device come first, so they can be exercised with a NULL handle; that one is refused last
    if (!gram) return fail(TI_E_ARG, "gram is NULL");
    if (!omega) return fail(TI_E_ARG, "omega is NULL");
    if (!g) return fail(TI_E_ARG, "g is NULL");
    if (!ev) return fail(TI_E_ARG, "ev is NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (g->p < 1) return fail(TI_E_ARG, "p must be >= 1");
    if (g->p > TI_EIGH_MAX_N) return fail(TI_E_UNSUPPORTED, "p must be <= 64 on the device: use the host route (observables.gedmd_spectrum, solver=\"host\")");
    if (g->d < 1 || g->d > 16) return fail(TI_E_ARG, "d must be in 1..16");
    if (g->nev < 1 || g->nev > g->p) return fail(TI_E_ARG, "nev must be in 1..p");
    if (g->reserved != 0) return fail(TI_E_ARG, "reserved must be 0");
    if (!std::isfinite(g->a)) return fail(TI_E_ARG, "a must be finite");
    if (!(std::isfinite(g->tol) && g->tol >= 0.0)) return fail(TI_E_ARG, "tol must be finite and >= 0");
    for (int i = 0; i < g->d * g->p; ++i)
        if (!std::isfinite(omega[i])) return fail(TI_E_ARG, "non-finite omega at entry " + std::to_string(i));
    if (int rc = eig_n_mat_refusal(n_mat)) return rc;
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const int d = g->d, p = g->p, nev = g->nev;
        const size_t pp = (size_t)p * p * 2, N = (size_t)n_mat, pv = (size_t)p * nev * 2;
        std::vector<double> K((size_t)p * p, 0.0);                  // K = omega^T omega, i ascending
        for (int i = 0; i < d; ++i)
            for (int k = 0; k < p; ++k)
                for (int l = 0; l < p; ++l) K[(size_t)k * p + l] += omega[i * p + k] * omega[i * p + l];
        h->eig_k.upload(K);
        Staged sg(h, mem);
        const double* gd = sg.in(gram, h->eig_a, N * pp);
        // matrices per launch: the eigenvectors and reduced matrices of a launch stay within 3 x 32 MiB whatever n_mat is
        const size_t chunk = std::min<size_t>(N, 512);
        grow(h->eig_w, chunk * p); grow(h->eig_v, chunk * pp); grow(h->eig_w2, chunk * p); grow(h->eig_v2, chunk * pp); grow(h->eig_r, chunk * pp);
        grow(h->eig_st, N); grow(h->eig_st2, N); grow(h->eig_rank, N); grow(h->eig_ev, N * nev);
        if (vec) grow(h->eig_vec, N * pv);
        for (size_t m0 = 0; m0 < N; m0 += chunk) {
            const long long nm = (long long)std::min(chunk, N - m0);
            int32_t *st1 = h->eig_st.p + m0, *st2 = h->eig_st2.p + m0, *rk = h->eig_rank.p + m0;
            HIP_CHECK(launch_obs_eigh(gd + m0 * pp, (long long)pp, p, p, nullptr, h->eig_w.p, h->eig_v.p, p, st1, nm, st));
            HIP_CHECK(launch_obs_gedmd_reduce(gd + m0 * pp, h->eig_w.p, h->eig_v.p, st1, h->eig_k.p, -0.5 * g->a, g->tol, nev, p, h->eig_r.p, rk, nm, st));
            HIP_CHECK(launch_obs_eigh(h->eig_r.p, (long long)pp, p, p, rk, h->eig_w2.p, h->eig_v2.p, p, st2, nm, st));
            HIP_CHECK(launch_obs_gedmd_back(h->eig_w.p, h->eig_v.p, h->eig_w2.p, h->eig_v2.p, st2, rk, nev, p, h->eig_ev.p + m0 * nev,
                                            vec ? h->eig_vec.p + m0 * pv : nullptr, nm, st));
        }
        std::vector<int32_t> s1(N), s2(N);
        HIP_CHECK(hipMemcpyAsync(s1.data(), h->eig_st.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(s2.data(), h->eig_st2.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (int rc = eig_status_refusal(s1, "Gram matrix")) return rc;
        for (auto& s : s2) s = s < 0 ? 1 : s;                      // a refused reduced matrix is the degenerate input: NaN, not an error
        if (int rc = eig_status_refusal(s2, "the reduced matrix of Gram matrix")) return rc;
        const hipMemcpyKind kind = mem == TI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        HIP_CHECK(hipMemcpyAsync(ev, h->eig_ev.p, N * nev * sizeof(double), kind, st));
        if (vec) HIP_CHECK(hipMemcpyAsync(vec, h->eig_vec.p, N * pv * sizeof(double), kind, st));
        if (rank) HIP_CHECK(hipMemcpyAsync(rank, h->eig_rank.p, N * sizeof(int32_t), kind, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return TI_OK;
    });
}

int64_t ti_obs_eigh_wide_launch_max(int32_t n) { return eigw_launch_max(n); }

// The blocked solve of nm <= eigw_launch_max(n) matrices of order n (or nvec [i] <= n; below 65 skipped): w [nm][ldo], v [nm][ldo][ldo][2]
// or NULL, status [nm] (device) as the narrow kernel leaves them.  The host reads the status words once per outer sweep and stops
// launching when no matrix is still iterating.
static void eigw_solve(ti_handle* h, const double* a, long long mat_stride, int lda, int n, const int* nvec, double* w, double* v, int ldo,
                       int32_t* status, long long nm)
{
    hipStream_t st = h->stream;
    const size_t N = (size_t)nm, nn = (size_t)n * n * 2, nslot = (size_t)eigw_slots(n) / 2, blk = (size_t)EIGW_PAIR * EIGW_PAIR * 2;
    grow(h->eigw_a, N * nn); grow(h->eigw_v, N * nn);
    grow(h->eigw_u, N * nslot * blk); grow(h->eigw_s, N * nslot * blk);
    grow(h->eigw_thr, N); grow(h->eigw_rot, N); grow(h->eigw_prot, N * nslot);
    EigWide e{};
    e.n = n; e.nvec = nvec; e.n_mat = nm;
    e.A = h->eigw_a.p; e.V = h->eigw_v.p; e.U = h->eigw_u.p; e.S = h->eigw_s.p;
    e.thr = h->eigw_thr.p; e.rot = h->eigw_rot.p; e.prot = h->eigw_prot.p; e.status = status;
    HIP_CHECK(launch_eigw_init(e, a, mat_stride, lda, st));
    std::vector<int32_t> hs(N);
    const int rounds = eigw_slots(n) - 1;
    for (int sweep = 1; sweep <= EIG_MAX_SWEEPS; ++sweep) {
        for (int r = 0; r < rounds; ++r) HIP_CHECK(launch_eigw_round(e, r, st));
        HIP_CHECK(launch_eigw_sweep_end(e, sweep, st));
        HIP_CHECK(hipMemcpyAsync(hs.data(), status, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (std::none_of(hs.begin(), hs.end(), [](int32_t s) { return s == 0; })) break;
    }
    HIP_CHECK(launch_eigw_finish(e, w, v, ldo, st));
}

int ti_obs_eigh_wide(ti_handle* h, const double* a, int64_t n_mat, int32_t n, double* w, double* v, int32_t* sweeps, int mem)
{
    // the checks that need no device come first, so they can be exercised with a NULL handle; that one is refused last
    if (!a) return fail(TI_E_ARG, "a is NULL");
    if (!w) return fail(TI_E_ARG, "w is NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n < 1 || n > TI_EIGH_WIDE_MAX_N) return fail(TI_E_ARG, "n must be in 1..1024");
    if (int rc = eig_n_mat_refusal(n_mat)) return rc;
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (n <= TI_EIGH_MAX_N) return ti_obs_eigh(h, a, n_mat, n, w, v, sweeps, mem);
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const size_t nn = (size_t)n * n * 2, N = (size_t)n_mat, chunk = (size_t)eigw_launch_max(n);
        Staged sg(h, mem);
        const double* ad = sg.in(a, h->eig_a, N * nn);
        grow(h->eig_w, N * n);
        if (v) grow(h->eig_v, N * nn);
        grow(h->eig_st, N);
        for (size_t m0 = 0; m0 < N; m0 += chunk)
            eigw_solve(h, ad + m0 * nn, (long long)nn, n, n, nullptr, h->eig_w.p + m0 * n, v ? h->eig_v.p + m0 * nn : nullptr, n, h->eig_st.p + m0,
                       (long long)std::min(chunk, N - m0));
        std::vector<int32_t> status(N);
        HIP_CHECK(hipMemcpyAsync(status.data(), h->eig_st.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (int rc = eig_status_refusal(status, "matrix")) return rc;
        const hipMemcpyKind kind = mem == TI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        HIP_CHECK(hipMemcpyAsync(w, h->eig_w.p, N * n * sizeof(double), kind, st));
        if (v) HIP_CHECK(hipMemcpyAsync(v, h->eig_v.p, N * nn * sizeof(double), kind, st));
        if (sweeps && mem == TI_MEM_DEVICE) HIP_CHECK(hipMemcpyAsync(sweeps, h->eig_st.p, N * sizeof(int32_t), kind, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (sweeps && mem == TI_MEM_HOST) std::copy(status.begin(), status.end(), sweeps);
        return TI_OK;
    });
}

int ti_obs_gedmd_spectrum_wide(ti_handle* h, const double* gram, int64_t n_mat, const double* omega, const ti_gedmd_desc* g, double* ev,
                               double* vec, int32_t* rank, int mem)
{
    // p <= 64 is the narrow call: its checks, its kernels, its bits
    if (!g || g->p <= TI_EIGH_MAX_N) return ti_obs_gedmd_spectrum(h, gram, n_mat, omega, g, ev, vec, rank, mem);
    if (!gram) return fail(TI_E_ARG, "gram is NULL");
    if (!omega) return fail(TI_E_ARG, "omega is NULL");
    if (!ev) return fail(TI_E_ARG, "ev is NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (g->p > TI_EIGH_WIDE_MAX_N) return fail(TI_E_UNSUPPORTED, "p must be <= 1024 on the device: use the host route (observables.gedmd_spectrum, solver=\"host\")");
    if (g->d < 1 || g->d > 16) return fail(TI_E_ARG, "d must be in 1..16");
    if (g->nev < 1 || g->nev > g->p) return fail(TI_E_ARG, "nev must be in 1..p");
    if (g->reserved != 0) return fail(TI_E_ARG, "reserved must be 0");
    if (!std::isfinite(g->a)) return fail(TI_E_ARG, "a must be finite");
    if (!(std::isfinite(g->tol) && g->tol >= 0.0)) return fail(TI_E_ARG, "tol must be finite and >= 0");
    for (int i = 0; i < g->d * g->p; ++i)
        if (!std::isfinite(omega[i])) return fail(TI_E_ARG, "non-finite omega at entry " + std::to_string(i));
    if (int rc = eig_n_mat_refusal(n_mat)) return rc;
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const int d = g->d, p = g->p, nev = g->nev;
        const size_t pp = (size_t)p * p * 2, N = (size_t)n_mat, pv = (size_t)p * nev * 2;
        std::vector<double> K((size_t)p * p, 0.0);                  // K = omega^T omega, i ascending
        for (int i = 0; i < d; ++i)
            for (int k = 0; k < p; ++k)
                for (int l = 0; l < p; ++l) K[(size_t)k * p + l] += omega[i * p + k] * omega[i * p + l];
        h->eig_k.upload(K);
        Staged sg(h, mem);
        const double* gd = sg.in(gram, h->eig_a, N * pp);
        const size_t chunk = std::min<size_t>(N, (size_t)eigw_launch_max(p));
        grow(h->eig_w, chunk * p); grow(h->eig_v, chunk * pp); grow(h->eig_w2, chunk * p); grow(h->eig_v2, chunk * pp); grow(h->eig_r, chunk * pp);
        grow(h->eigw_sv, chunk * p); grow(h->eigw_l, chunk * pp); grow(h->eigw_t, chunk * pp);
        grow(h->eigw_nvn, chunk); grow(h->eigw_nvw, chunk); grow(h->eigw_live, chunk);
        grow(h->eig_st, N); grow(h->eig_st2, N); grow(h->eigw_st2n, N); grow(h->eig_rank, N); grow(h->eig_ev, N * nev);
        if (vec) grow(h->eig_vec, N * pv);
        std::vector<int32_t> rk_host(chunk);
        for (size_t m0 = 0; m0 < N; m0 += chunk) {
            const long long nm = (long long)std::min(chunk, N - m0);
            int32_t *st1 = h->eig_st.p + m0, *st2n = h->eigw_st2n.p + m0, *st2w = h->eig_st2.p + m0, *rk = h->eig_rank.p + m0;
            eigw_solve(h, gd + m0 * pp, (long long)pp, p, p, nullptr, h->eig_w.p, h->eig_v.p, p, st1, nm);
            HIP_CHECK(launch_eigw_gedmd_rank(h->eig_w.p, h->eig_v.p, st1, g->tol, nev, p, h->eigw_sv.p, h->eigw_l.p, h->eig_r.p, rk, h->eigw_nvn.p,
                                             h->eigw_nvw.p, h->eigw_live.p, nm, st));
            HIP_CHECK(launch_eigw_gedmd_reduce(gd + m0 * pp, h->eig_k.p, -0.5 * g->a, h->eigw_l.p, rk, h->eigw_live.p, p, h->eigw_t.p, h->eig_r.p, nm, st));
            // the second solve: orders up to 64 by ti_obs_eigh's kernel, the others by the blocked one sized for the largest rank
            HIP_CHECK(launch_obs_eigh(h->eig_r.p, (long long)pp, p, EIG_MAX_N, h->eigw_nvn.p, h->eig_w2.p, h->eig_v2.p, p, st2n, nm, st));
            HIP_CHECK(hipMemcpyAsync(rk_host.data(), rk, (size_t)nm * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            const int rmax = *std::max_element(rk_host.begin(), rk_host.begin() + nm);
            if (rmax > EIG_MAX_N) eigw_solve(h, h->eig_r.p, (long long)pp, p, rmax, h->eigw_nvw.p, h->eig_w2.p, h->eig_v2.p, p, st2w, nm);
            else HIP_CHECK(hipMemsetAsync(st2w, 0, (size_t)nm * sizeof(int32_t), st));
            HIP_CHECK(launch_eigw_gedmd_back(h->eigw_l.p, h->eig_w2.p, h->eig_v2.p, st2n, st2w, rk, nev, p, h->eig_ev.p + m0 * nev,
                                             vec ? h->eig_vec.p + m0 * pv : nullptr, nm, st));
        }
        std::vector<int32_t> s1(N), s2(N), s2n(N);
        HIP_CHECK(hipMemcpyAsync(s1.data(), h->eig_st.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(s2.data(), h->eig_st2.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(s2n.data(), h->eigw_st2n.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (int rc = eig_status_refusal(s1, "Gram matrix")) return rc;
        for (size_t i = 0; i < N; ++i) { s2[i] += s2n[i]; s2[i] = s2[i] < 0 ? 1 : s2[i]; }      // a refused reduced matrix is the degenerate input: NaN, not an error
        if (int rc = eig_status_refusal(s2, "the reduced matrix of Gram matrix")) return rc;
        const hipMemcpyKind kind = mem == TI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        HIP_CHECK(hipMemcpyAsync(ev, h->eig_ev.p, N * nev * sizeof(double), kind, st));
        if (vec) HIP_CHECK(hipMemcpyAsync(vec, h->eig_vec.p, N * pv * sizeof(double), kind, st));
        if (rank) HIP_CHECK(hipMemcpyAsync(rank, h->eig_rank.p, N * sizeof(int32_t), kind, st));
        HIP_CHECK(hipStreamSynchronize(st));
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
        const float *vd = values, *ld = logw;
        long long sd = stride;
        if (mem == TI_MEM_HOST) {                      // the column only: B floats, not B * stride
            grow(h->obs_val, (size_t)B);
            std::vector<float> col((size_t)B);
            for (int64_t i = 0; i < B; ++i) col[i] = values[i * stride];
            HIP_CHECK(hipMemcpy(h->obs_val.p, col.data(), (size_t)B * sizeof(float), hipMemcpyHostToDevice));
            vd = h->obs_val.p; sd = 1;
        }
        if (logw) ld = Staged(h, mem).in(logw, h->obs_logw, (size_t)B);
        double norm[4];
        if (logw) { if (int rc = obs_norm_dev(h, ld, B, norm)) return rc; }
        else {
            grow(h->obs_red, 4 + 259);
            grow(h->obs_part, (size_t)OBS_MAX_BLOCKS * 259);
        }
        HIP_CHECK(launch_obs_whist(h->obs_red.p + 4, h->obs_part.p, vd, sd, ld, h->obs_red.p, B, n_bins, lo, hi, st));
        std::vector<double> out((size_t)n_bins + 3);
        HIP_CHECK(hipMemcpyAsync(out.data(), h->obs_red.p + 4, out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::copy(out.begin(), out.begin() + n_bins, out_hist);
        std::copy(out.begin() + n_bins, out.end(), out_tails);
        return TI_OK;
    });
}

int ti_obs_ff_set(ti_handle* h, const ti_ff_desc* desc, const int32_t* bond_idx, const double* bond_par, const int32_t* angle_idx,
                  const double* angle_par, const int32_t* torsion_idx, const double* torsion_par, const double* pair_par)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (!desc) { h->ff_on = false; h->ff_mass_on = false; return TI_OK; }
    if (!h->natoms.empty()) return fail(TI_E_UNSUPPORTED, "one force field is one species: clear ti_painn_set_molecules first");
    const int A = h->d.n_atoms;
    const int n[4] = {desc->n_bonds, desc->n_angles, desc->n_torsions, desc->n_pairs};
    const int cap[4] = {TI_FF_MAX_BONDS, TI_FF_MAX_ANGLES, TI_FF_MAX_TORSIONS, TI_FF_MAX_PAIRS};
    const char* name[4] = {"bond", "angle", "torsion", "pair"};
    const int32_t* idx[3] = {bond_idx, angle_idx, torsion_idx};
    const double* par[4] = {bond_par, angle_par, torsion_par, pair_par};
    for (int t = 0; t < 4; ++t) {
        if (n[t] < 0 || n[t] > cap[t]) return fail(TI_E_ARG, std::string(name[t]) + " count " + std::to_string(n[t]) + " is outside 0.." + std::to_string(cap[t]));
        if (n[t] > 0 && (!par[t] || (t < 3 && !idx[t]))) return fail(TI_E_ARG, std::string(name[t]) + " table is NULL");
    }
    if (n[3] != A * (A - 1) / 2) return fail(TI_E_ARG, "the pair table must hold all A (A - 1) / 2 = " + std::to_string(A * (A - 1) / 2) + " pairs, got " + std::to_string(n[3]));
    if (!std::isfinite(desc->coulomb)) return fail(TI_E_ARG, "coulomb must be finite");
    std::vector<int32_t> words; std::vector<double> pars;
    for (int t = 0; t < 3; ++t) {                              // bonds (2 atoms, 2 parameters), angles (3, 2), torsions (4, 3)
        const int na = 2 + t, np = t == 2 ? 3 : 2;
        for (int k = 0; k < n[t]; ++k) {
            const std::string what = std::string(name[t]) + " " + std::to_string(k);
            const int32_t* a = idx[t] + (size_t)na * k;
            const double* q = par[t] + (size_t)np * k;
            int32_t w = 0;
            for (int s = 0; s < na; ++s) {
                if (a[s] < 0 || a[s] >= A) return fail(TI_E_ARG, what + ": atom index outside 0.." + std::to_string(A - 1));
                for (int s2 = 0; s2 < s; ++s2)
                    if (a[s2] == a[s]) return fail(TI_E_ARG, what + ": atom " + std::to_string(a[s]) + " is repeated");
                w |= a[s] << (5 * s);
            }
            for (int s = 0; s < np; ++s)
                if (!std::isfinite(q[s])) return fail(TI_E_ARG, what + ": non-finite parameter");
            if (t == 2) {                                      // (n, phase, k): the periodicity goes into the word
                if (q[0] != std::floor(q[0]) || q[0] < 1.0 || q[0] > 6.0) return fail(TI_E_ARG, what + ": the periodicity must be an integer in 1..6");
                w |= (int32_t)q[0] << 20;
                pars.push_back(q[1]); pars.push_back(q[2]);
            } else {
                pars.push_back(q[0]); pars.push_back(q[1]);
            }
            words.push_back(w);
        }
    }
    for (int i = 0, k = 0; i < A; ++i)                         // row i (2A - i - 1) / 2 + (j - i - 1)
        for (int j = i + 1; j < A; ++j, ++k) {
            const double* q = pair_par + 3 * (size_t)k;
            const std::string what = "pair " + std::to_string(k) + " (" + std::to_string(i) + ", " + std::to_string(j) + ")";
            if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) return fail(TI_E_ARG, what + ": non-finite parameter");
            if (q[1] < 0.0 || q[2] < 0.0) return fail(TI_E_ARG, what + ": sigma and eps must be >= 0");
            words.push_back(i | j << 5 | ((q[0] != 0.0 || q[2] != 0.0) ? FF_LIVE : 0));
            pars.insert(pars.end(), q, q + 3);
        }
    const std::vector<int32_t> inc = ff_build_incidence(words, n, A);      // of the bonded terms, for ti_obs_ff_forces / ti_obs_ff_langevin
    return guarded([&]() -> int {
        set_device(h);
        h->ff_on = false;
        h->ff_mass_on = false;                                 // the masses go with the force field (ti_obs_ff_set_masses)
        h->ff_idx.upload(words);
        h->ff_par.upload(pars);
        h->ff_inc.upload(inc);
        std::copy(n, n + 4, h->ff_n);
        h->ff_coulomb = desc->coulomb;
        h->ff_on = true;
        return TI_OK;
    });
}

int ti_obs_ff_energy(ti_handle* h, const float* x, int64_t B, double to_nm, const float* T, double* out_e, double* out_terms, int mem)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (B < 0 || (B > 0 && (!x || !out_e))) return fail(TI_E_ARG, "NULL buffer");
    if (!std::isfinite(to_nm)) return fail(TI_E_ARG, "to_nm must be finite");
    if (!h->ff_on) return fail(TI_E_ARG, "no force field set (ti_obs_ff_set)");
    if (!h->natoms.empty()) return fail(TI_E_UNSUPPORTED, "one force field is one species: clear ti_painn_set_molecules first");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const int A = h->d.n_atoms;
        Staged sg(h, mem);
        const float* xd = sg.in(x, h->obs_x, (size_t)B * 3 * A);
        const float* Td = T ? sg.in(T, h->ff_T, (size_t)B) : nullptr;
        if (Td) {                                      // refused before anything is written, the index found as ti_obs_weights finds its own
            grow(h->obs_red, 4 + 259);
            double bad = 0.0;
            HIP_CHECK(launch_obs_ff_bad_temperature(h->obs_red.p, Td, B, st));
            HIP_CHECK(hipMemcpyAsync(&bad, h->obs_red.p, sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (bad < (double)B) return fail(TI_E_ARG, "T must be finite and > 0: index " + std::to_string((long long)bad));
        }
        FfParams p{};
        p.x = xd; p.T = Td; p.B = B; p.A = A; p.to_nm = to_nm; p.coulomb = h->ff_coulomb;
        p.nb = h->ff_n[0]; p.na = h->ff_n[1]; p.nt = h->ff_n[2]; p.np = h->ff_n[3];
        p.idx = h->ff_idx.p; p.par = h->ff_par.p;
        p.e = sg.out(out_e, h->ff_e, (size_t)B);
        p.terms = out_terms ? sg.out(out_terms, h->ff_terms, (size_t)B * 4) : nullptr;
        HIP_CHECK(launch_obs_ff_energy(p, st));
        sg.finish();
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
        grow(h->obs_red, 4 + 259);
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

// The checks ti_obs_zmat and ti_obs_zmat_xyz share, all before any device work; on TI_OK `topo` holds order [A] then ref [A][3].
static int zmat_check(ti_handle* h, const int32_t* order, const int32_t* ref, int mem, std::vector<int32_t>& topo)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    const int A = h->d.n_atoms;
    if (A < 2 || A > ZMAT_MAX_ATOMS) return fail(TI_E_ARG, "a Z-matrix needs 2 <= A <= " + std::to_string(ZMAT_MAX_ATOMS) + ", the handle has A = " + std::to_string(A));
    if (!h->natoms.empty()) return fail(TI_E_UNSUPPORTED, "one topology is one species: clear ti_painn_set_molecules first");
    if (!ref) return fail(TI_E_ARG, "ref is NULL");
    topo.assign((size_t)4 * A, 0);
    std::vector<char> seen((size_t)A, 0);
    for (int s = 0; s < A; ++s) {
        const int a = order ? order[s] : s;
        if (a < 0 || a >= A || seen[a]) return fail(TI_E_ARG, "order is not a permutation of 0.." + std::to_string(A - 1) + " (entry " + std::to_string(s) + ")");
        seen[a] = 1;
        topo[s] = a;
    }
    for (int s = 1; s < A; ++s) {
        const int n = s < 3 ? s : 3;                           // the slots that are read
        for (int j = 0; j < n; ++j) {
            const int r = ref[3 * s + j];
            if (r < 0 || r >= s) return fail(TI_E_ARG, "ref[" + std::to_string(s) + "][" + std::to_string(j) + "] = " + std::to_string(r) + " is not an earlier sorted atom");
            for (int j2 = 0; j2 < j; ++j2)
                if (ref[3 * s + j2] == r) return fail(TI_E_ARG, "ref[" + std::to_string(s) + "] repeats atom " + std::to_string(r));
            topo[A + 3 * s + j] = r;
        }
    }
    return TI_OK;
}

int ti_obs_zmat(ti_handle* h, const int32_t* order, const int32_t* ref, const float* x, int64_t B, float* out_z, int mem)
{
    std::vector<int32_t> topo;
    if (int rc = zmat_check(h, order, ref, mem, topo)) return rc;
    if (B < 0 || (B > 0 && (!x || !out_z))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        const int A = h->d.n_atoms;
        h->zm_topo.upload(topo);
        Staged sg(h, mem);
        ZmatParams p{};
        p.x = sg.in(x, h->obs_x, (size_t)B * 3 * A);
        p.B = B; p.A = A; p.topo = h->zm_topo.p;
        p.z = sg.out(out_z, h->zm_z, (size_t)B * 3 * (A - 1));
        HIP_CHECK(launch_obs_zmat(p, h->stream));
        sg.finish();
        return TI_OK;
    });
}

int ti_obs_zmat_xyz(ti_handle* h, const int32_t* order, const int32_t* ref, const float* z, int64_t B, float* out_x, double* out_logdet,
                    uint8_t* out_valid, int mem)
{
    std::vector<int32_t> topo;
    if (int rc = zmat_check(h, order, ref, mem, topo)) return rc;
    if (B < 0 || (B > 0 && (!z || !out_x))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        const int A = h->d.n_atoms;
        h->zm_topo.upload(topo);
        Staged sg(h, mem);
        ZmatXyzParams p{};
        p.z = sg.in(z, h->zm_z, (size_t)B * 3 * (A - 1));
        p.B = B; p.A = A; p.topo = h->zm_topo.p;
        p.x = sg.out(out_x, h->obs_x, (size_t)B * 3 * A);
        p.logdet = out_logdet ? sg.out(out_logdet, h->zm_logdet, (size_t)B) : nullptr;
        p.valid = out_valid ? sg.out(out_valid, h->zm_valid, (size_t)B) : nullptr;
        HIP_CHECK(launch_obs_zmat_xyz(p, h->stream));
        sg.finish();
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
        grow(h->obs_red, 4 + std::max<size_t>((size_t)K * ncol, 259));          // at least what obs_norm_dev asks for: it must not move them
        grow(h->obs_part, (size_t)OBS_MAX_BLOCKS * std::max<size_t>((size_t)K * ncol, 259));
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

}  // extern "C"
