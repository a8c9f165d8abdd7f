// api_obs_eig.hip -- C ABI of the batched Hermitian eigensolvers and of the gEDMD spectra on them (include/ti_hip.h ti_obs_eigh,
// ti_obs_eigh_wide, ti_obs_gedmd_spectrum, ti_obs_gedmd_spectrum_wide): checks, staging, the cut into launches and the status
// refusals.  Kernels: obs_eig_kernels.hip (orders up to 64, in LDS), obs_eig_wide_kernels.hip (blocked, orders 65..1024).
#include "ti_handle.hpp"

// the refusals found in the status words of a solve over n_mat matrices (host copy)
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

// The refusals of an eigensolver entry (max_n: TI_EIGH_MAX_N or TI_EIGH_WIDE_MAX_N).  Those that need no device come first, so
// they can be exercised with a NULL handle; that one is refused last.
static int eigh_refusal(const ti_handle* h, const double* a, int64_t n_mat, int32_t n, const double* w, int mem, int max_n)
{
    if (!a) return fail(TI_E_ARG, "a is NULL");
    if (!w) return fail(TI_E_ARG, "w is NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n < 1 || n > max_n) return fail(TI_E_ARG, "n must be in 1.." + std::to_string(max_n));
    if (int rc = eig_n_mat_refusal(n_mat)) return rc;
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return TI_OK;
}

// The body of both eigensolver entries after their checks: staging, the solve, the status refusal, the copy-out.
// solve(ad) enqueues the solve of all n_mat matrices at ad into h->eig_w, h->eig_v (when v is asked for) and h->eig_st.
template <typename Solve>
static int eigh_call(ti_handle* h, const double* a, int64_t n_mat, int32_t n, double* w, double* v, int32_t* sweeps, int mem, Solve&& solve)
{
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const size_t nn = (size_t)n * n * 2, N = (size_t)n_mat;
        Staged sg(h, mem);
        const double* ad = sg.in(a, h->eig_a, N * nn);
        grow(h->eig_w, N * n);
        if (v) grow(h->eig_v, N * nn);
        grow(h->eig_st, N);
        solve(ad);
        std::vector<int32_t> status(N);
        HIP_CHECK(hipMemcpyAsync(status.data(), h->eig_st.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (int rc = eig_status_refusal(status, "matrix")) return rc;
        HIP_CHECK(hipMemcpyAsync(w, h->eig_w.p, N * n * sizeof(double), out_kind(mem), st));
        if (v) HIP_CHECK(hipMemcpyAsync(v, h->eig_v.p, N * nn * sizeof(double), out_kind(mem), st));
        if (sweeps && mem == TI_MEM_DEVICE) HIP_CHECK(hipMemcpyAsync(sweeps, h->eig_st.p, N * sizeof(int32_t), out_kind(mem), st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (sweeps && mem == TI_MEM_HOST) std::copy(status.begin(), status.end(), sweeps);      // the words are here already
        return TI_OK;
    });
}

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

// The refusals of a spectrum entry (max_p: TI_EIGH_MAX_N or TI_EIGH_WIDE_MAX_N).  Those that need no device come first, so they
// can be exercised with a NULL handle; that one is refused last.
static int gedmd_refusal(const ti_handle* h, const double* gram, int64_t n_mat, const double* omega, const ti_gedmd_desc* g, const double* ev,
                         int mem, int max_p)
{
    if (!gram) return fail(TI_E_ARG, "gram is NULL");
    if (!omega) return fail(TI_E_ARG, "omega is NULL");
    if (!g) return fail(TI_E_ARG, "g is NULL");
    if (!ev) return fail(TI_E_ARG, "ev is NULL");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (g->p < 1) return fail(TI_E_ARG, "p must be >= 1");
    if (g->p > max_p)
        return fail(TI_E_UNSUPPORTED, "p must be <= " + std::to_string(max_p) + " on the device: use the host route (observables.gedmd_spectrum, solver=\"host\")");
    if (g->d < 1 || g->d > 16) return fail(TI_E_ARG, "d must be in 1..16");
    if (g->nev < 1 || g->nev > g->p) return fail(TI_E_ARG, "nev must be in 1..p");
    if (g->reserved != 0) return fail(TI_E_ARG, "reserved must be 0");
    if (!std::isfinite(g->a)) return fail(TI_E_ARG, "a must be finite");
    if (!(std::isfinite(g->tol) && g->tol >= 0.0)) return fail(TI_E_ARG, "tol must be finite and >= 0");
    for (int i = 0; i < g->d * g->p; ++i)
        if (!std::isfinite(omega[i])) return fail(TI_E_ARG, "non-finite omega at entry " + std::to_string(i));
    if (int rc = eig_n_mat_refusal(n_mat)) return rc;
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return TI_OK;
}

// K = omega^T omega (i ascending) into h->eig_k
static void gedmd_upload_k(ti_handle* h, const double* omega, int d, int p)
{
    std::vector<double> K((size_t)p * p, 0.0);
    for (int i = 0; i < d; ++i)
        for (int k = 0; k < p; ++k)
            for (int l = 0; l < p; ++l) K[(size_t)k * p + l] += omega[i * p + k] * omega[i * p + l];
    h->eig_k.upload(K);
}

// The end of a spectrum call over N matrices: the status words of the first solve (h->eig_st) and of the second (h->eig_st2, plus
// st2_more [N] when a second kernel took part of them; NULL: none) with their refusals, then ev, vec and rank to the caller.
static int gedmd_finish(ti_handle* h, size_t N, int nev, size_t pv, const int32_t* st2_more, double* ev, double* vec, int32_t* rank, int mem)
{
    hipStream_t st = h->stream;
    std::vector<int32_t> s1(N), s2(N), s2m(st2_more ? N : 0);
    HIP_CHECK(hipMemcpyAsync(s1.data(), h->eig_st.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(s2.data(), h->eig_st2.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (st2_more) HIP_CHECK(hipMemcpyAsync(s2m.data(), st2_more, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (int rc = eig_status_refusal(s1, "Gram matrix")) return rc;
    for (size_t i = 0; i < N; ++i) {                               // a refused reduced matrix is the degenerate input: NaN, not an error
        if (st2_more) s2[i] += s2m[i];
        s2[i] = s2[i] < 0 ? 1 : s2[i];
    }
    if (int rc = eig_status_refusal(s2, "the reduced matrix of Gram matrix")) return rc;
    HIP_CHECK(hipMemcpyAsync(ev, h->eig_ev.p, N * nev * sizeof(double), out_kind(mem), st));
    if (vec) HIP_CHECK(hipMemcpyAsync(vec, h->eig_vec.p, N * pv * sizeof(double), out_kind(mem), st));
    if (rank) HIP_CHECK(hipMemcpyAsync(rank, h->eig_rank.p, N * sizeof(int32_t), out_kind(mem), st));
    HIP_CHECK(hipStreamSynchronize(st));
    return TI_OK;
}

extern "C" {

int ti_obs_eigh(ti_handle* h, const double* a, int64_t n_mat, int32_t n, double* w, double* v, int32_t* sweeps, int mem)
{
    if (int rc = eigh_refusal(h, a, n_mat, n, w, mem, TI_EIGH_MAX_N)) return rc;
    return eigh_call(h, a, n_mat, n, w, v, sweeps, mem, [&](const double* ad) {
        HIP_CHECK(launch_obs_eigh(ad, (long long)n * n * 2, n, n, nullptr, h->eig_w.p, v ? h->eig_v.p : nullptr, n, h->eig_st.p, n_mat, h->stream));
    });
}

int64_t ti_obs_eigh_wide_launch_max(int32_t n) { return eigw_launch_max(n); }

int ti_obs_eigh_wide(ti_handle* h, const double* a, int64_t n_mat, int32_t n, double* w, double* v, int32_t* sweeps, int mem)
{
    if (int rc = eigh_refusal(h, a, n_mat, n, w, mem, TI_EIGH_WIDE_MAX_N)) return rc;
    if (n <= TI_EIGH_MAX_N) return ti_obs_eigh(h, a, n_mat, n, w, v, sweeps, mem);
    return eigh_call(h, a, n_mat, n, w, v, sweeps, mem, [&](const double* ad) {
        const size_t nn = (size_t)n * n * 2, N = (size_t)n_mat, chunk = (size_t)eigw_launch_max(n);
        for (size_t m0 = 0; m0 < N; m0 += chunk)
            eigw_solve(h, ad + m0 * nn, (long long)nn, n, n, nullptr, h->eig_w.p + m0 * n, v ? h->eig_v.p + m0 * nn : nullptr, n, h->eig_st.p + m0,
                       (long long)std::min(chunk, N - m0));
    });
}

int ti_obs_gedmd_spectrum(ti_handle* h, const double* gram, int64_t n_mat, const double* omega, const ti_gedmd_desc* g, double* ev, double* vec,
                          int32_t* rank, int mem)
{
    if (int rc = gedmd_refusal(h, gram, n_mat, omega, g, ev, mem, TI_EIGH_MAX_N)) return rc;
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const int p = g->p, nev = g->nev;
        const size_t pp = (size_t)p * p * 2, N = (size_t)n_mat, pv = (size_t)p * nev * 2;
        gedmd_upload_k(h, omega, g->d, p);
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
        return gedmd_finish(h, N, nev, pv, nullptr, ev, vec, rank, mem);
    });
}

int ti_obs_gedmd_spectrum_wide(ti_handle* h, const double* gram, int64_t n_mat, const double* omega, const ti_gedmd_desc* g, double* ev,
                               double* vec, int32_t* rank, int mem)
{
    // p <= 64 is the narrow call: its checks, its kernels, its bits
    if (!g || g->p <= TI_EIGH_MAX_N) return ti_obs_gedmd_spectrum(h, gram, n_mat, omega, g, ev, vec, rank, mem);
    if (int rc = gedmd_refusal(h, gram, n_mat, omega, g, ev, mem, TI_EIGH_WIDE_MAX_N)) return rc;
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const int p = g->p, nev = g->nev;
        const size_t pp = (size_t)p * p * 2, N = (size_t)n_mat, pv = (size_t)p * nev * 2;
        gedmd_upload_k(h, omega, g->d, p);
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
        return gedmd_finish(h, N, nev, pv, h->eigw_st2n.p, ev, vec, rank, mem);
    });
}

}  // extern "C"
