// api_obs_tica.hip -- C ABI of TICA (include/ti_hip.h ti_obs_tica_moments, ti_obs_tica_fit, ti_obs_tica_transform): checks, the pair
// counts, staging, the cut into launches and the status refusals.  Kernels: obs_tica_kernels.hip, and obs_eig_kernels.hip for the
// two solves.
#include "ti_handle.hpp"

static int tica_feature_dim(int K, int encode) { return encode ? 2 * K : K; }

// the refusals of the strided values of a TICA call; d: the caller's feature count, or -1 to take it from (K, encode)
static int tica_values_refusal(const float* values, int64_t stride, int64_t cstride, int64_t n, int32_t K, int32_t encode, int d, int mem)
{
    if (!values) return fail(TI_E_ARG, "values is NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (encode != 0 && encode != 1) return fail(TI_E_ARG, "encode must be 0 or 1");
    if (K < 1 || K > TI_TICA_MAX_K) return fail(TI_E_ARG, "K must be in 1.." + std::to_string(TI_TICA_MAX_K));
    if (tica_feature_dim(K, encode) > TI_EIGH_MAX_N) return fail(TI_E_ARG, "d must be <= " + std::to_string(TI_EIGH_MAX_N));
    if (d >= 0 && d != tica_feature_dim(K, encode)) return fail(TI_E_ARG, "d must be K (encode = 0) or 2 K (encode = 1)");
    if (n < 1 || n > (int64_t)INT32_MAX) return fail(TI_E_ARG, "the row count must be in 1..2^31-1");
    if (cstride < 1) return fail(TI_E_ARG, "cstride must be >= 1");
    if (cstride > (int64_t)INT32_MAX || stride < (K - 1) * cstride + 1) return fail(TI_E_ARG, "stride must be >= (K - 1) cstride + 1");
    return TI_OK;
}

// The K columns of the n rows of p.  TI_MEM_HOST: packed densely into b, so that only they cross the bus, and the strides become (K, 1).
static const float* tica_values_in(int mem, const float* p, long long& stride, long long& cstride, long long n, int K, DevBuf<float>& b)
{
    if (mem != TI_MEM_HOST) return p;
    std::vector<float> rows((size_t)n * K);
    for (long long i = 0; i < n; ++i)
        for (int k = 0; k < K; ++k) rows[(size_t)i * K + k] = p[i * stride + k * cstride];
    grow(b, rows.size());
    HIP_CHECK(hipMemcpy(b.p, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
    stride = K;
    cstride = 1;
    return b.p;
}

extern "C" {

int ti_obs_tica_moments(ti_handle* h, const float* values, int64_t stride, int64_t cstride, int64_t n, int32_t K, int32_t encode,
                        const int64_t* traj_off, int64_t n_traj, const int32_t* lags, int32_t n_lag, int64_t* count, double* sum, double* cov,
                        int mem)
{
    // the checks that need no device come first, so they can be exercised with a NULL handle; that one is refused last
    if (int rc = tica_values_refusal(values, stride, cstride, n, K, encode, -1, mem)) return rc;
    if (!traj_off || !lags || !count || !sum || !cov) return fail(TI_E_ARG, "NULL buffer");
    if (n_lag < 1 || n_lag > TI_TICA_MAX_LAGS) return fail(TI_E_ARG, "n_lag must be in 1.." + std::to_string(TI_TICA_MAX_LAGS));
    if (n_traj < 1 || n_traj > n) return fail(TI_E_ARG, "n_traj must be in 1..n");
    if (traj_off[0] != 0 || traj_off[n_traj] != n) return fail(TI_E_ARG, "traj_off must start at 0 and end at n");
    for (int64_t t = 0; t < n_traj; ++t)
        if (traj_off[t + 1] <= traj_off[t]) return fail(TI_E_ARG, "traj_off must be strictly ascending (entry " + std::to_string(t + 1) + ")");
    // the cumulative pair counts of every lag
    const size_t nt1 = (size_t)n_traj + 1;
    std::vector<long long> cum((size_t)n_lag * nt1, 0);
    for (int l = 0; l < n_lag; ++l) {
        if (lags[l] < 1) return fail(TI_E_ARG, "lag " + std::to_string(l) + " must be >= 1");
        long long* c = cum.data() + (size_t)l * nt1;
        for (int64_t t = 0; t < n_traj; ++t) c[t + 1] = c[t] + std::max<long long>(traj_off[t + 1] - traj_off[t] - lags[l], 0);
        if (c[n_traj] < 2)
            return fail(TI_E_ARG, "lag " + std::to_string(lags[l]) + " (entry " + std::to_string(l) + ") has " + std::to_string(c[n_traj]) + " pairs: at least 2 are needed");
    }
    if (!h) return fail(TI_E_ARG, "NULL handle");
    const int d = tica_feature_dim(K, encode), D = gram_pad(d), T = D / 16;
    if (n * D > ((int64_t)1 << 27)) return fail(TI_E_ALLOC, "the feature table would exceed 1 GiB (n * D > 2^27, D = d rounded up to 16)");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        long long sd = stride, cd = cstride;
        const float* xd = tica_values_in(mem, values, sd, cd, n, K, h->tica_x);
        h->tica_off.upload(std::vector<long long>(traj_off, traj_off + nt1));
        grow(h->tica_f, (size_t)n * D);
        grow(h->tica_bad, (size_t)tica_feature_blocks(n, encode, D) + 1);
        long long* first_bad = h->tica_bad.p + tica_feature_blocks(n, encode, D);
        HIP_CHECK(launch_tica_features(h->tica_f.p, h->tica_bad.p, first_bad, xd, sd, cd, n, K, encode, D, st));
        // a non-finite value is refused before anything is contracted
        long long bad = 0;
        HIP_CHECK(hipMemcpyAsync(&bad, first_bad, sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (bad != LLONG_MAX) return fail(TI_E_NAN, "non-finite value in row " + std::to_string(bad));
        grow(h->tica_sum, (size_t)n_lag * 2 * d);
        grow(h->tica_cov, (size_t)n_lag * 3 * d * d);
        // lags per launch: the partial tiles of a launch stay within 256 MiB (one lag always fits: at most 2^27 / 16 / 8192 segments)
        const size_t part_doubles = (size_t)tica_tiles(T) * 256, max_segs = ((size_t)256 << 20) / (part_doubles * 8);
        std::vector<long long> counts(n_lag);
        for (int l0 = 0; l0 < n_lag;) {
            TicaParams g{};
            g.f = h->tica_f.p; g.traj_off = h->tica_off.p; g.n_traj = (int)n_traj;
            int nl = 0;
            while (l0 + nl < n_lag) {
                const long long np = cum[(size_t)(l0 + nl) * nt1 + n_traj], nseg = (np + TICA_SEG - 1) / TICA_SEG;
                if (nl > 0 && (size_t)(g.seg_off[nl] + nseg) > max_segs) break;
                g.lag[nl] = lags[l0 + nl];
                g.seg_off[nl + 1] = g.seg_off[nl] + (int)nseg;
                counts[l0 + nl] = np;
                ++nl;
            }
            g.n_lag = nl;
            grow(h->tica_cum, (size_t)nl * nt1);
            // the stream is drained before the table of the launch before this one is overwritten
            HIP_CHECK(hipStreamSynchronize(st));
            HIP_CHECK(hipMemcpy(h->tica_cum.p, cum.data() + (size_t)l0 * nt1, (size_t)nl * nt1 * sizeof(long long), hipMemcpyHostToDevice));
            g.cum = h->tica_cum.p;
            grow(h->tica_part, (size_t)g.seg_off[nl] * part_doubles);
            g.part = h->tica_part.p;
            HIP_CHECK(launch_tica_moments(g, T, h->tica_sum.p + (size_t)l0 * 2 * d, h->tica_cov.p + (size_t)l0 * 3 * d * d, d, st));
            l0 += nl;
        }
        static_assert(sizeof(long long) == sizeof(int64_t), "count is copied as it stands");
        if (mem == TI_MEM_HOST) std::copy(counts.begin(), counts.end(), count);
        else HIP_CHECK(hipMemcpyAsync(count, counts.data(), (size_t)n_lag * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(sum, h->tica_sum.p, (size_t)n_lag * 2 * d * sizeof(double), out_kind(mem), st));
        HIP_CHECK(hipMemcpyAsync(cov, h->tica_cov.p, (size_t)n_lag * 3 * d * d * sizeof(double), out_kind(mem), st));
        HIP_CHECK(hipStreamSynchronize(st));
        return TI_OK;
    });
}

int ti_obs_tica_fit(ti_handle* h, const int64_t* count, const double* sum, const double* cov, int32_t n_lag, int32_t d, const ti_tica_desc* desc,
                    double* mean, double* ev, double* comp, int32_t* rank, int mem)
{
    if (!count || !sum || !cov || !desc || !mean || !ev || !comp || !rank) return fail(TI_E_ARG, "NULL buffer");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n_lag < 1 || n_lag > TI_TICA_MAX_LAGS) return fail(TI_E_ARG, "n_lag must be in 1.." + std::to_string(TI_TICA_MAX_LAGS));
    if (d < 1 || d > TI_EIGH_MAX_N) return fail(TI_E_ARG, "d must be in 1.." + std::to_string(TI_EIGH_MAX_N));
    if (desc->dim < 1 || desc->dim > d) return fail(TI_E_ARG, "dim must be in 1..d");
    if (desc->scaling != 0 && desc->scaling != 1) return fail(TI_E_ARG, "scaling must be 0 or 1 (kinetic map)");
    if (desc->reserved != 0) return fail(TI_E_ARG, "reserved must be 0");
    if (!(std::isfinite(desc->epsilon) && desc->epsilon >= 0.0)) return fail(TI_E_ARG, "epsilon must be finite and >= 0");
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const int dim = desc->dim;
        const size_t N = (size_t)n_lag, dd = (size_t)d * d;
        std::vector<long long> counts(N);
        if (mem == TI_MEM_HOST) std::copy(count, count + N, counts.begin());
        else {
            HIP_CHECK(hipMemcpyAsync(counts.data(), count, N * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        for (size_t l = 0; l < N; ++l)
            if (counts[l] < 2) return fail(TI_E_ARG, "count " + std::to_string(l) + " is " + std::to_string(counts[l]) + ": at least 2 pairs are needed");
        Staged sg(h, mem);
        const long long* cd = reinterpret_cast<const long long*>(count);
        if (mem == TI_MEM_HOST) { h->tica_cnt.upload(counts); cd = h->tica_cnt.p; }
        const double* sd = sg.in(sum, h->tica_sum, N * 2 * d);
        const double* vd = sg.in(cov, h->tica_cov, N * 3 * dd);
        grow(h->eig_a, N * dd * 2); grow(h->eig_w, N * d); grow(h->eig_v, N * dd * 2); grow(h->eig_w2, N * d); grow(h->eig_v2, N * dd * 2);
        grow(h->eig_r, N * dd * 2); grow(h->eig_st, N); grow(h->eig_st2, N); grow(h->eig_rank, N);
        grow(h->tica_c0t, N * dd); grow(h->tica_l, N * dd); grow(h->tica_flag, N);
        grow(h->tica_mean, N * d); grow(h->tica_ev, N * dim); grow(h->tica_comp, N * d * dim);
        HIP_CHECK(launch_tica_fit_prep(cd, sd, vd, d, h->tica_mean.p, h->eig_a.p, h->tica_c0t.p, h->tica_flag.p, n_lag, st));
        HIP_CHECK(launch_obs_eigh(h->eig_a.p, (long long)dd * 2, d, d, nullptr, h->eig_w.p, h->eig_v.p, d, h->eig_st.p, n_lag, st));
        HIP_CHECK(launch_tica_fit_reduce(h->eig_w.p, h->eig_v.p, h->eig_st.p, h->tica_c0t.p, desc->epsilon, d, h->tica_l.p, h->eig_r.p, h->eig_rank.p,
                                         n_lag, st));
        HIP_CHECK(launch_obs_eigh(h->eig_r.p, (long long)dd * 2, d, d, h->eig_rank.p, h->eig_w2.p, h->eig_v2.p, d, h->eig_st2.p, n_lag, st));
        HIP_CHECK(launch_tica_fit_back(h->tica_l.p, h->eig_w2.p, h->eig_v2.p, h->eig_rank.p, d, dim, desc->scaling, h->tica_ev.p, h->tica_comp.p,
                                       n_lag, st));
        std::vector<int32_t> flag(N), s1(N), s2(N);
        HIP_CHECK(hipMemcpyAsync(flag.data(), h->tica_flag.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(s1.data(), h->eig_st.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(s2.data(), h->eig_st2.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (size_t l = 0; l < N; ++l) {
            if (flag[l] || s1[l] < 0 || s2[l] < 0) return fail(TI_E_NAN, "non-finite moment of lag entry " + std::to_string(l));
            if (s1[l] > EIG_MAX_SWEEPS || s2[l] > EIG_MAX_SWEEPS)
                return fail(TI_E_UNSUPPORTED, "a matrix of lag entry " + std::to_string(l) + " is still rotating after " + std::to_string(EIG_MAX_SWEEPS) + " sweeps");
        }
        HIP_CHECK(hipMemcpyAsync(mean, h->tica_mean.p, N * d * sizeof(double), out_kind(mem), st));
        HIP_CHECK(hipMemcpyAsync(ev, h->tica_ev.p, N * dim * sizeof(double), out_kind(mem), st));
        HIP_CHECK(hipMemcpyAsync(comp, h->tica_comp.p, N * d * dim * sizeof(double), out_kind(mem), st));
        HIP_CHECK(hipMemcpyAsync(rank, h->eig_rank.p, N * sizeof(int32_t), out_kind(mem), st));
        HIP_CHECK(hipStreamSynchronize(st));
        return TI_OK;
    });
}

int ti_obs_tica_transform(ti_handle* h, const float* values, int64_t stride, int64_t cstride, int64_t B, int32_t K, int32_t encode,
                          const double* mean, const double* comp, int32_t n_lag, int32_t d, int32_t dim, float* out, int mem)
{
    if (int rc = tica_values_refusal(values, stride, cstride, B, K, encode, d, mem)) return rc;
    if (!mean || !comp || !out) return fail(TI_E_ARG, "NULL buffer");
    if (n_lag < 1 || n_lag > TI_TICA_MAX_LAGS) return fail(TI_E_ARG, "n_lag must be in 1.." + std::to_string(TI_TICA_MAX_LAGS));
    if (dim < 1 || dim > d) return fail(TI_E_ARG, "dim must be in 1..d");
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        long long sd = stride, cd = cstride;
        const float* xd = tica_values_in(mem, values, sd, cd, B, K, h->tica_x);
        Staged sg(h, mem);
        const double* md = sg.in(mean, h->tica_mean, (size_t)n_lag * d);
        const double* pd = sg.in(comp, h->tica_comp, (size_t)n_lag * d * dim);
        float* od = sg.out(out, h->tica_y, (size_t)n_lag * (size_t)B * dim);
        HIP_CHECK(launch_tica_transform(od, xd, sd, cd, B, K, encode, d, dim, md, pd, n_lag, st));
        sg.finish();
        return TI_OK;
    });
}

}  // extern "C"
