// rollout.hpp -- the integrator drivers of libti_hip.so on top of a drift callable: the fixed-step schemes (rollout_common), the
// Runge-Kutta schemes restating torchdiffeq 0.2.5 (rollout_rk), dopri5 with per-trajectory step control (rollout_rk_traj), and what
// they share (second state of the dlogp ODE, mixed-species batches, the attached observer, the final-state check).  Templates on the
// drift callable: included by the units that instantiate them (api_painn.hip, api_adw.hip).
#pragma once
#include "ti_handle.hpp"

namespace ti {

// drift(x_dev, t, out_dev) evaluates the drift; state arrays have n floats; comps = floats per trajectory
// Optional second state of the reference ODE: d(dlogp)/dt = -div * 1e-2, returned * 1e2 (adw/thermo/integrators.py:38-68).
struct DlogpAux {
    float *dl = nullptr, *d1 = nullptr, *d2 = nullptr, *scaled = nullptr, *out = nullptr;
    size_t n_dl = 0;                              // entries of the second state (0: same as the first state's n)
    float div_scale = 1e-2f, out_scale = 100.0f;  // d(dlogp)/dt = -div_scale * div, written * out_scale
};

// Mixed-species batches (ti_painn_set_molecules): device atom counts [B] of a state [B][A][3], and the number of real floats in it.
// n == NULL: every entry is real.  The drift already returns +0 on pad atoms, so the fixed-step updates leave them where they are;
// what changes is the EM noise, the adaptive solvers' norms and their dense output.
struct Ragged { const int32_t* n = nullptr; int A = 0; size_t n_real = 0; };
inline Ragged ragged_of(const ti_handle* h) { return h->ragged ? Ragged{h->natoms_dev.p, h->d.n_atoms, (size_t)h->n_real * 3} : Ragged{}; }

// The attached observer of a rollout over B trajectories: at(i, x) writes the CV row of grid point i when the observer wants one.
struct Observer {
    ti_handle* h; long long B; int N; int64_t row = 0;
    bool on() const { return h->obs[1].K > 0; }
    bool wants(int i) const { return on() && (h->obs_every > 0 ? (i % h->obs_every == 0 || i == N - 1) : i == N - 1); }
    void at(int i, const float* x_dev)
    {
        if (!wants(i)) return;
        const size_t nk = (size_t)B * h->obs[1].K;
        float* dst = h->obs_out + (size_t)(row++) * nk;
        if (h->obs_mem == TI_MEM_DEVICE) { obs_cv_dev(h, 1, x_dev, B, dst); return; }
        grow(h->obs_cv, nk);
        obs_cv_dev(h, 1, x_dev, B, h->obs_cv.p);
        HIP_CHECK(hipMemcpyAsync(dst, h->obs_cv.p, nk * sizeof(float), hipMemcpyDeviceToHost, h->stream));     // pageable: done on return
    }
};

// The end of every rollout: TI_E_NAN if the final state x [n] holds a non-finite value.  Synchronises the handle's stream.
inline int final_state_check(ti_handle* h, const float* x, size_t n)
{
    hipStream_t st = h->stream;
    HIP_CHECK(hipMemsetAsync(h->nanflag.p, 0, sizeof(int), st));
    HIP_CHECK(launch_nan_check(x, (long long)n, h->nanflag.p, st));
    int flag = 0;
    HIP_CHECK(hipMemcpyAsync(&flag, h->nanflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return flag ? fail(TI_E_NAN, "non-finite value in the final state") : TI_OK;
}

template <typename Drift>
int rollout_common(ti_handle* h, const ti_rollout_desc* rd, float* x, float* b1, float* b2, float* xt, size_t n, long long B, int comps,
                   int atoms_for_com, float* out_path, int64_t* n_fevals, Drift&& drift, DlogpAux aux = DlogpAux(), Ragged rg = Ragged())
{
    hipStream_t st = h->stream;
    const hipMemcpyKind out_kind = rd->mem == TI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    int64_t row = 0, fe = 0;
    const size_t ndl = aux.n_dl ? aux.n_dl : n;
    if (aux.dl) HIP_CHECK(hipMemsetAsync(aux.dl, 0, ndl * sizeof(float), st));
    auto save = [&]() {
        if (aux.dl) {
            HIP_CHECK(launch_scale(aux.scaled, aux.dl, aux.out_scale, (long long)ndl, st));
            HIP_CHECK(hipMemcpyAsync(aux.out + (size_t)row * ndl, aux.scaled, ndl * sizeof(float), out_kind, st));
        }
        HIP_CHECK(hipMemcpyAsync(out_path + (size_t)(row++) * n, x, n * sizeof(float), out_kind, st));
    };
    Observer obs{h, B, rd->n_step};
    if (rd->save_every > 0) save();
    if (obs.on()) obs.at(0, x);
    for (int k = 0; k < rd->n_step - 1; ++k) {
        const float dt = rd->t_grid[k + 1] - rd->t_grid[k];
        drift(x, rd->t_grid[k], b1, aux.d1); ++fe;
        if (rd->scheme == TI_SCHEME_HEUN) {
            { Timed tm(h, TI_KERNEL_INTEGRATE); HIP_CHECK(launch_axpy(xt, x, dt, b1, (long long)n, st)); }
            drift(xt, rd->t_grid[k + 1], b2, aux.d2); ++fe;
            { Timed tm(h, TI_KERNEL_INTEGRATE); HIP_CHECK(launch_heun(x, 0.5f * dt, b1, b2, (long long)n, st)); }
            if (aux.dl) HIP_CHECK(launch_heun(aux.dl, -0.5f * dt * aux.div_scale, aux.d1, aux.d2, (long long)ndl, st));
        } else {
            Timed tm(h, TI_KERNEL_INTEGRATE);
            HIP_CHECK(launch_axpy(x, x, dt, b1, (long long)n, st));
            if (aux.dl) HIP_CHECK(launch_axpy(aux.dl, aux.dl, -dt * aux.div_scale, aux.d1, (long long)ndl, st));
            if (rd->scheme == TI_SCHEME_EM && rd->eps > 0.0f && rg.n)
                HIP_CHECK(launch_noise_ragged(x, std::sqrt(2.0f * rd->eps * std::fabs(dt)), rd->seed, rd->traj_offset, (int)(rd->step_offset + k), B, rg.A,
                                              rd->com_free_noise ? 1 : 0, rg.n, st));
            else if (rd->scheme == TI_SCHEME_EM && rd->eps > 0.0f)
                HIP_CHECK(launch_noise(x, std::sqrt(2.0f * rd->eps * std::fabs(dt)), rd->seed, rd->traj_offset, (int)(rd->step_offset + k), B, comps,
                                       rd->com_free_noise ? atoms_for_com : 0, st));
        }
        const int step = k + 1;
        if (rd->save_every > 0 && (step % rd->save_every == 0 || step == rd->n_step - 1)) save();
        if (obs.on()) obs.at(step, x);
    }
    if (rd->save_every <= 0) save();
    if (n_fevals) *n_fevals = fe;
    return final_state_check(h, x, n);
}

// ---- Runge-Kutta drivers on top of the same drift callback: torchdiffeq 0.2.5's `dopri5` (adaptive), `midpoint`, `rk4`
// (include/ti_hip.h TI_SCHEME_*).  State = segment 0 (x, n floats) and optionally segment 1 (dlogp, aux.n_dl floats) with
// right-hand side (b, -div_scale * div); a decreasing grid is integrated in s = -t with f'(s, y) = -f(-s, y) like
// torchdiffeq's _ReverseFunc.  Times and step sizes are fp64 on the host and enter state arithmetic as fp32, as there.
namespace dp5 {
constexpr double alpha[6] = {1. / 5, 3. / 10, 4. / 5, 8. / 9, 1., 1.};
constexpr double beta[6][6] = {{1. / 5},
                               {3. / 40, 9. / 40},
                               {44. / 45, -56. / 15, 32. / 9},
                               {19372. / 6561, -25360. / 2187, 64448. / 6561, -212. / 729},
                               {9017. / 3168, -355. / 33, 46732. / 5247, 49. / 176, -5103. / 18656},
                               {35. / 384, 0., 500. / 1113, 125. / 192, -2187. / 6784, 11. / 84}};
constexpr double c_error[7] = {35. / 384 - 1951. / 21600, 0., 500. / 1113 - 22642. / 50085, 125. / 192 - 451. / 720,
                               -2187. / 6784 - -12231. / 42400, 11. / 84 - 649. / 6300, -1. / 60};
constexpr double c_mid[7] = {6025192743. / 30085553152. / 2, 0., 51252292925. / 65400821598. / 2, -2691868925. / 45128329728. / 2,
                             187940372067. / 1594534317056. / 2, -1776094331. / 19743644256. / 2, 11237099. / 235043384. / 2};
}  // namespace dp5

template <typename Drift>
int rollout_rk(ti_handle* h, const ti_rollout_desc* rd, float* x, size_t n, float* out_path, int64_t* n_fevals, Drift&& drift,
               DlogpAux aux = DlogpAux(), Ragged rg = Ragged())
{
    hipStream_t st = h->stream;
    const hipMemcpyKind out_kind = rd->mem == TI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const int nseg = aux.dl ? 2 : 1;
    const size_t ndl = aux.dl ? (aux.n_dl ? aux.n_dl : n) : 0;
    const size_t sn[2] = {n, ndl};
    // workspace: per segment k[7], ytmp, ynew, coef[5]
    const size_t per = 14;
    grow(h->rk_ws, per * (n + ndl));
    grow(h->rk_red, (size_t)RED_PARTIALS + 8);
    float* y[2] = {x, aux.dl};
    float *k[2][7] = {}, *ytmp[2] = {}, *ynew[2] = {}, *coef[2] = {};
    struct Pair { float* p[2]; operator float* const*() const { return p; } };
    auto KP = [&](int j) { return Pair{{k[0][j], k[1][j]}}; };
    {
        float* w = h->rk_ws.p;
        for (int s2 = 0; s2 < nseg; ++s2) {
            for (int j = 0; j < 7; ++j) { k[s2][j] = w; w += sn[s2]; }
            ytmp[s2] = w; w += sn[s2]; ynew[s2] = w; w += sn[s2]; coef[s2] = w; w += 5 * sn[s2];
        }
    }
    if (aux.dl) HIP_CHECK(hipMemsetAsync(aux.dl, 0, ndl * sizeof(float), st));
    const int N = rd->n_step;
    const double sign = (N > 1 && rd->t_grid[1] < rd->t_grid[0]) ? -1.0 : 1.0;
    int64_t fe = 0, row = 0;
    // f(s, y) for every segment; `ti` is the fp32 stage time in the (possibly negated) integration variable
    auto F = [&](float ti, float* const* yin, float* const* kout) {
        drift(yin[0], (float)(sign * (double)ti), kout[0], aux.dl ? aux.d1 : nullptr); ++fe;
        if (aux.dl) HIP_CHECK(launch_scale(kout[1], aux.d1, (float)(-sign) * aux.div_scale, (long long)ndl, st));
        if (sign < 0) HIP_CHECK(launch_scale(kout[0], kout[0], -1.0f, (long long)n, st));
    };
    auto save_from = [&](float* const* src) {
        if (aux.dl) {
            HIP_CHECK(launch_scale(aux.scaled, src[1], aux.out_scale, (long long)ndl, st));
            HIP_CHECK(hipMemcpyAsync(aux.out + (size_t)row * ndl, aux.scaled, ndl * sizeof(float), out_kind, st));
        }
        HIP_CHECK(hipMemcpyAsync(out_path + (size_t)(row++) * n, src[0], n * sizeof(float), out_kind, st));
    };
    auto wants_row = [&](int i) { return rd->save_every > 0 ? (i % rd->save_every == 0 || i == N - 1) : i == N - 1; };
    auto comb = [&](int s2, int nk, const double* c, double scale) {
        RkComb r{};
        r.nk = nk;
        for (int j = 0; j < nk; ++j) { r.k[j] = k[s2][j]; r.c[j] = (float)c[j] * (float)scale; }       // beta_ij * dt in fp32
        return r;
    };
    double* red = h->rk_red.p;
    auto fetch = [&]() { double v = 0; HIP_CHECK(hipMemcpyAsync(&v, red + RED_PARTIALS, sizeof(double), hipMemcpyDeviceToHost, st)); HIP_CHECK(hipStreamSynchronize(st)); return v; };
    const float rtol = rd->rtol, atol = rd->atol;
    Observer obs{h, (long long)(n / (size_t)obs_floats_per_traj(h)), N};
    if (wants_row(0)) save_from(y);
    if (obs.on()) obs.at(0, y[0]);

    if (rd->scheme == TI_SCHEME_MIDPOINT || rd->scheme == TI_SCHEME_RK4) {
        // FixedGridODESolver with step_size = None: one step per grid interval (solvers.py; fixed_grid.py Midpoint / RK4)
        for (int i = 0; i + 1 < N; ++i) {
            const float t0 = (float)(sign * rd->t_grid[i]), t1 = (float)(sign * rd->t_grid[i + 1]), dt = t1 - t0;
            F(t0, y, KP(0));
            if (rd->scheme == TI_SCHEME_MIDPOINT) {
                const double half[1] = {0.5};
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 1, half, dt), (long long)sn[s2], st));
                F(t0 + 0.5f * dt, ytmp, KP(1));
                const double one[2] = {0., 1.};
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(y[s2], y[s2], comb(s2, 2, one, dt), (long long)sn[s2], st));
            } else {                        // rk4_alt_step_func: the 3/8 rule
                const double c2[1] = {1. / 3}, c3[2] = {-1. / 3, 1.}, c4[3] = {1., -1., 1.}, cs[4] = {0.125, 0.375, 0.375, 0.125};
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 1, c2, dt), (long long)sn[s2], st));
                F(t0 + dt * (1.0f / 3.0f), ytmp, KP(1));
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 2, c3, dt), (long long)sn[s2], st));
                F(t0 + dt * (2.0f / 3.0f), ytmp, KP(2));
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 3, c4, dt), (long long)sn[s2], st));
                F(t1, ytmp, KP(3));
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(y[s2], y[s2], comb(s2, 4, cs, dt), (long long)sn[s2], st));
            }
            if (wants_row(i + 1)) save_from(y);
            if (obs.on()) obs.at(i + 1, y[0]);
        }
    } else {
        // ---- dopri5: RKAdaptiveStepsizeODESolver (rk_common.py) ----
        auto norm_of = [&](auto&& launch_one) {        // mixed norm: max over segments of the rms (misc.py _mixed_norm / _rms_norm)
            double best = 0.0;
            for (int s2 = 0; s2 < nseg; ++s2) {
                launch_one(s2);
                best = std::max(best, std::sqrt(fetch() / (double)(s2 == 0 && rg.n ? rg.n_real : sn[s2])));      // rms over the real entries
            }
            return best;
        };
        const double t_first = sign * (double)rd->t_grid[0];
        F((float)t_first, y, KP(0));
        // _select_initial_step(func, t0, y0, order - 1 = 4, rtol, atol, norm, f0)
        // segment 0 of a mixed-species batch takes the ragged sums (pad entries skipped)
        auto scaled_sumsq = [&](int s2, const float* a, const float* b2) {
            if (s2 == 0 && rg.n) HIP_CHECK(launch_scaled_sumsq_ragged(red + RED_PARTIALS, red, a, b2, y[s2], rtol, atol, (long long)sn[s2], rg.n, 3 * rg.A, st));
            else HIP_CHECK(launch_scaled_sumsq(red + RED_PARTIALS, red, a, b2, y[s2], rtol, atol, (long long)sn[s2], st));
        };
        const double d0 = norm_of([&](int s2) { scaled_sumsq(s2, y[s2], nullptr); });
        const double d1 = norm_of([&](int s2) { scaled_sumsq(s2, k[s2][0], nullptr); });
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        {
            const double one[1] = {1.};
            for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_rk_combo(ytmp[s2], y[s2], comb(s2, 1, one, h0), (long long)sn[s2], st));
        }
        F((float)(t_first + h0), ytmp, KP(1));
        const double d2 = norm_of([&](int s2) { scaled_sumsq(s2, k[s2][1], k[s2][0]); }) / h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3) : std::pow(0.01 / std::max(d1, d2), 1.0 / 5.0);
        double dt = std::min(100.0 * h0, h1);
        double t0 = t_first, t1 = t_first;            // interpolation interval of the last accepted step
        long long attempts = 0;
        for (int i = 1; i < N; ++i) {
            const double next_t = sign * (double)rd->t_grid[i];
            while (next_t > t1) {
                if (++attempts > 10000000LL) return fail(TI_E_NAN, "dopri5: more than 1e7 step attempts");
                const double ts = t1, te = ts + dt;
                if (!(te > ts)) return fail(TI_E_NAN, "dopri5: step size underflow (dt = " + std::to_string(dt) + ")");
                const float tsf = (float)ts, dtf = (float)dt, tef = (float)te;
                for (int sidx = 0; sidx < 6; ++sidx) {                       // _runge_kutta_step
                    const float ti = dp5::alpha[sidx] == 1.0 ? std::nextafterf(tef, tef - 1.0f) : tsf + (float)dp5::alpha[sidx] * dtf;
                    float* const* dst = sidx == 5 ? ynew : ytmp;             // c_sol == beta[5]: the last stage input IS y1
                    for (int s2 = 0; s2 < nseg; ++s2)
                        HIP_CHECK(launch_rk_combo(dst[s2], y[s2], comb(s2, sidx + 1, dp5::beta[sidx], dtf), (long long)sn[s2], st));
                    F(ti, dst, KP(sidx + 1));
                }
                const double ratio = norm_of([&](int s2) {                  // _compute_error_ratio
                    if (s2 == 0 && rg.n) HIP_CHECK(launch_rk_ratio_sumsq_ragged(red + RED_PARTIALS, red, y[s2], ynew[s2], comb(s2, 7, dp5::c_error, dtf), rtol, atol, (long long)sn[s2], rg.n, 3 * rg.A, st));
                    else HIP_CHECK(launch_rk_ratio_sumsq(red + RED_PARTIALS, red, y[s2], ynew[s2], comb(s2, 7, dp5::c_error, dtf), rtol, atol, (long long)sn[s2], st));
                });
                if (!(ratio == ratio)) return fail(TI_E_NAN, "dopri5: non-finite error estimate");
                if (ratio <= 1.0) {                                          // accept: dense output, FSAL
                    for (int s2 = 0; s2 < nseg; ++s2) {
                        HIP_CHECK(launch_interp_fit(coef[s2], y[s2], ynew[s2], k[s2][0], k[s2][6], comb(s2, 7, dp5::c_mid, dtf), dtf, (long long)sn[s2], st));
                        HIP_CHECK(hipMemcpyAsync(y[s2], ynew[s2], sn[s2] * sizeof(float), hipMemcpyDeviceToDevice, st));
                        std::swap(k[s2][0], k[s2][6]);
                    }
                    t0 = ts; t1 = te;
                }
                // _optimal_step_size(dt, ratio, safety 0.9, ifactor 10, dfactor 0.2, order 5)
                if (ratio == 0.0) dt *= 10.0;
                else dt *= std::min(10.0, std::max(0.9 / std::pow(ratio, 0.2), ratio < 1.0 ? 1.0 : 0.2));
            }
            if (wants_row(i)) {                                              // _interp_evaluate at the requested time
                const float xrel = (float)((next_t - t0) / (t1 - t0));
                for (int s2 = 0; s2 < nseg; ++s2) HIP_CHECK(launch_interp_eval(ytmp[s2], coef[s2], xrel, (long long)sn[s2], st));
                if (rg.n) HIP_CHECK(launch_copy_pads(ytmp[0], y[0], rg.n, (long long)(n / (3 * rg.A)), rg.A, 3, st));      // pads: the state, not its fit
                save_from(ytmp);
                if (obs.on()) obs.at(i, ytmp[0]);
            } else if (obs.wants(i)) {                                       // an observer row where no path row is written: x only
                const float xrel = (float)((next_t - t0) / (t1 - t0));
                HIP_CHECK(launch_interp_eval(ytmp[0], coef[0], xrel, (long long)sn[0], st));
                obs.at(i, ytmp[0]);
            }
        }
    }
    if (n_fevals) *n_fevals = fe;
    return final_state_check(h, x, n);
}

// ---- dopri5 with per-trajectory step control (TI_SCHEME_DOPRI5_TRAJ): trajectory b of m floats (plus its dlogp entry) runs the
// algorithm of rollout_rk above on its own -- initial step from its own norms, its own accept / reject decisions, step sizes and
// dense output (ode_kernels.hip, TrajRkParams) -- inside batched drift launches that take one stage time per trajectory
// (drift(x, tv, out, out_div), tv a device array [B]).  The batch takes as many attempts as its hardest trajectory; a finished
// (frozen) trajectory is evaluated along but never written again.  One small status read-back per attempt, as in rollout_rk.
template <typename DriftTv>
int rollout_rk_traj(ti_handle* h, const ti_rollout_desc* rd, float* x, long long B, long long m, float* out_path, int64_t* n_fevals,
                    DriftTv&& drift, DlogpAux aux = DlogpAux(), Ragged rg = Ragged())
{
    hipStream_t st = h->stream;
    const int nseg = aux.dl ? 2 : 1, N = rd->n_step;
    const size_t n = (size_t)B * m, ndl = aux.dl ? (size_t)B : 0, sn[2] = {n, ndl};
    const size_t per = 14;                                   // per segment k[7], ytmp, ynew, coef[5]
    grow(h->rk_ws, per * (n + ndl));
    grow(h->rk_ctl, (size_t)B);
    grow(h->rk_tv, (size_t)B);
    grow(h->rk_status, (size_t)TRAJ_ST_N);
    const int total_rows = (int)ti_rollout_rows(N, rd->save_every);
    const bool host_out = rd->mem == TI_MEM_HOST;            // rows are written on the device and copied out as they complete
    float* path_dev = out_path;
    float* dl_dev = aux.out;
    if (host_out) {
        grow(h->rk_path, (size_t)total_rows * n);
        path_dev = h->rk_path.p;
        if (aux.dl) { grow(h->rk_dpath, (size_t)total_rows * ndl); dl_dev = h->rk_dpath.p; }
    }
    const double sign = (N > 1 && rd->t_grid[1] < rd->t_grid[0]) ? -1.0 : 1.0;
    {
        std::vector<double> g(N);
        for (int i = 0; i < N; ++i) g[i] = sign * (double)rd->t_grid[i];
        h->rk_grid.upload(g);
    }
    TrajRkParams p{};
    p.nseg = nseg; p.B = B; p.ctl = h->rk_ctl.p; p.tv = h->rk_tv.p; p.status = h->rk_status.p; p.grid = h->rk_grid.p;
    p.n_grid = N; p.save_every = rd->save_every; p.total_rows = total_rows; p.sign = sign; p.t_first = sign * (double)rd->t_grid[0];
    p.rtol = rd->rtol; p.atol = rd->atol; p.max_attempts = 10000000LL;
    {
        float* w = h->rk_ws.p;
        float* y[2] = {x, aux.dl};
        for (int s2 = 0; s2 < nseg; ++s2) {
            TrajSeg& g = p.seg[s2];
            for (int j = 0; j < 7; ++j) { g.k[j] = w; w += sn[s2]; }
            g.ytmp = w; w += sn[s2]; g.ynew = w; w += sn[s2]; g.coef = w; w += 5 * sn[s2];
            g.y = y[s2]; g.m = s2 ? 1 : m; g.out = s2 ? dl_dev : path_dev; g.out_scale = s2 ? aux.out_scale : 1.0f;
        }
    }
    if (aux.dl) HIP_CHECK(hipMemsetAsync(aux.dl, 0, ndl * sizeof(float), st));
    int64_t fe = 0;
    auto F = [&](int which) {                                // k[which] = f(s, y_in) at the stage times in rk_tv
        float* yin[2] = {which == 0 ? p.seg[0].y : which == 6 ? p.seg[0].ynew : p.seg[0].ytmp,
                         aux.dl ? (which == 0 ? p.seg[1].y : which == 6 ? p.seg[1].ynew : p.seg[1].ytmp) : nullptr};
        drift(yin[0], h->rk_tv.p, p.seg[0].k[which], aux.dl ? aux.d1 : nullptr); ++fe;
        if (aux.dl) HIP_CHECK(launch_scale(p.seg[1].k[which], aux.d1, (float)(-sign) * aux.div_scale, (long long)ndl, st));
        if (sign < 0) HIP_CHECK(launch_scale(p.seg[0].k[which], p.seg[0].k[which], -1.0f, (long long)n, st));
    };
    auto wants_row0 = rd->save_every > 0 || N == 1;
    if (wants_row0) {
        HIP_CHECK(hipMemcpyAsync(path_dev, x, n * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (aux.dl) HIP_CHECK(launch_scale(dl_dev, aux.dl, aux.out_scale, (long long)ndl, st));
    }
    {
        const float t0f = (float)(sign * (double)(float)p.t_first);
        uint32_t bits; std::memcpy(&bits, &t0f, 4);
        HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->rk_tv.p), (int)bits, (size_t)B, st));
    }
    F(0);
    HIP_CHECK(rg.n ? launch_traj_init_ragged(p, 0, rg.n, st) : launch_traj_init(p, 0, st));                    // _select_initial_step, per trajectory
    F(1);
    HIP_CHECK(rg.n ? launch_traj_init_ragged(p, 1, rg.n, st) : launch_traj_init(p, 1, st));
    float c_err[7], c_mid[7];
    for (int j = 0; j < 7; ++j) { c_err[j] = (float)dp5::c_error[j]; c_mid[j] = (float)dp5::c_mid[j]; }
    int status[TRAJ_ST_N] = {0, 0, INT_MAX, INT_MAX, INT_MAX, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(h->rk_status.p, status, sizeof(status), hipMemcpyHostToDevice, st));
    int copied = 0;                                           // rows already copied to the host
    auto copy_rows = [&](int upto) {
        if (!host_out || upto <= copied) return;
        HIP_CHECK(hipMemcpyAsync(out_path + (size_t)copied * n, path_dev + (size_t)copied * n, (size_t)(upto - copied) * n * sizeof(float),
                                 hipMemcpyDeviceToHost, st));
        if (aux.dl) HIP_CHECK(hipMemcpyAsync(aux.out + (size_t)copied * ndl, dl_dev + (size_t)copied * ndl, (size_t)(upto - copied) * ndl * sizeof(float),
                                             hipMemcpyDeviceToHost, st));
        copied = upto;
    };
    for (bool active = N > 1; active;) {
        HIP_CHECK(hipMemsetAsync(h->rk_status.p, 0, 2 * sizeof(int), st));        // active count, rows missing
        for (int sidx = 0; sidx < 6; ++sidx) {                                   // _runge_kutta_step, every trajectory with its own dt
            float c[6];
            for (int j = 0; j <= sidx; ++j) c[j] = (float)dp5::beta[sidx][j];
            HIP_CHECK(rg.n ? launch_traj_stage_ragged(p, c, sidx + 1, (float)dp5::alpha[sidx], dp5::alpha[sidx] == 1.0, sidx == 5, sidx == 0, rg.n, st)
                           : launch_traj_stage(p, c, sidx + 1, (float)dp5::alpha[sidx], dp5::alpha[sidx] == 1.0, sidx == 5, sidx == 0, st));
            F(sidx == 5 ? 6 : sidx + 1);
        }
        HIP_CHECK(rg.n ? launch_traj_advance_ragged(p, c_err, c_mid, rg.n, st) : launch_traj_advance(p, c_err, c_mid, st));
        HIP_CHECK(hipMemcpyAsync(status, h->rk_status.p, sizeof(status), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (status[TRAJ_ST_UNDERFLOW] != INT_MAX)
            return fail(TI_E_NAN, "dopri5 (per trajectory): step size underflow in trajectory " + std::to_string(status[TRAJ_ST_UNDERFLOW]));
        if (status[TRAJ_ST_NAN] != INT_MAX)
            return fail(TI_E_NAN, "dopri5 (per trajectory): non-finite error estimate in trajectory " + std::to_string(status[TRAJ_ST_NAN]));
        if (status[TRAJ_ST_LIMIT] != INT_MAX)
            return fail(TI_E_NAN, "dopri5 (per trajectory): more than 1e7 step attempts in trajectory " + std::to_string(status[TRAJ_ST_LIMIT]));
        copy_rows(total_rows - status[TRAJ_ST_MISSING]);                          // completed-row watermark
        active = status[TRAJ_ST_ACTIVE] > 0;
    }
    copy_rows(total_rows);
    std::vector<TrajCtl> ctl(B);
    HIP_CHECK(hipMemcpyAsync(ctl.data(), h->rk_ctl.p, (size_t)B * sizeof(TrajCtl), hipMemcpyDeviceToHost, st));
    const int rc = final_state_check(h, x, n);
    h->traj_accepted.resize(B); h->traj_rejected.resize(B);
    for (long long b = 0; b < B; ++b) { h->traj_accepted[b] = ctl[b].accepted; h->traj_rejected[b] = ctl[b].rejected; }
    if (n_fevals) *n_fevals = fe;
    return rc;
}

inline int check_rollout_desc(const ti_rollout_desc* rd)
{
    if (!rd || !rd->t_grid) return fail(TI_E_ARG, "rollout desc / t_grid is NULL");
    if (rd->n_step < 1) return fail(TI_E_ARG, "n_step must be >= 1");
    if (rd->scheme < TI_SCHEME_EULER || rd->scheme > TI_SCHEME_DOPRI5_TRAJ) return fail(TI_E_ARG, "unknown scheme");
    const bool adaptive = rd->scheme == TI_SCHEME_DOPRI5 || rd->scheme == TI_SCHEME_DOPRI5_TRAJ;
    if (adaptive && !(rd->rtol > 0.f && rd->atol > 0.f)) return fail(TI_E_ARG, "dopri5 needs rtol > 0 and atol > 0");
    if (rd->scheme >= TI_SCHEME_DOPRI5)
        for (int k = 0; k + 2 < rd->n_step; ++k)
            if ((rd->t_grid[k + 1] > rd->t_grid[k]) != (rd->t_grid[k + 2] > rd->t_grid[k + 1]) || rd->t_grid[k + 1] == rd->t_grid[k])
                return fail(TI_E_ARG, "t_grid must be strictly monotonic");
    if (rd->mem != TI_MEM_HOST && rd->mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem kind");
    if (rd->eps < 0.f) return fail(TI_E_ARG, "eps must be >= 0");
    if (rd->step_offset < 0 || rd->step_offset + rd->n_step > 0x7fffffffLL) return fail(TI_E_ARG, "step_offset out of range");
    return TI_OK;
}

}  // namespace ti
