// train_optim.hpp -- the optimiser shell the two trainers share (host only; included by api_adw_train.hip and api_painn_train.hip and
// nothing else): the Adam descriptor and its checks, the fp64 master state with its counters, clip + Adam with a given gradient, the
// state entry points' bodies, the read-back of a gradient call, and the index handling of a many-step call.  The kernels are those of
// adw_train_kernels.hip and vloss_kernels.hip.  What a trainer keeps for itself: its layers, arenas and staging buffers, its forward
// and backward pass, and its policy for the host mirror of the counters in a many-step call.
#pragma once
#include "ti_handle.hpp"
#include "adw_train.hpp"

namespace ti {
namespace {      // internal to either unit, as the copies this header replaced were: the library exports nothing new

constexpr int RED_LOSS = 0, RED_SUMSQ = 1;      // slots of Optim::red; a trainer may keep more behind them

struct AdamDesc { double lr, beta1, beta2, eps, weight_decay, max_grad_norm; };      // what ti_adw_train_desc and ti_painn_train_desc begin with

inline int lr_check(double lr) { return std::isfinite(lr) && lr > 0.0 ? TI_OK : fail(TI_E_ARG, "lr must be finite and > 0"); }

inline int adam_desc_check(const AdamDesc& t)
{
    if (int rc = lr_check(t.lr)) return rc;
    if (!(t.beta1 >= 0.0 && t.beta1 < 1.0) || !(t.beta2 >= 0.0 && t.beta2 < 1.0)) return fail(TI_E_ARG, "beta1 and beta2 must be in [0, 1)");
    if (!(std::isfinite(t.eps) && t.eps > 0.0)) return fail(TI_E_ARG, "eps must be finite and > 0");
    if (!(std::isfinite(t.weight_decay) && t.weight_decay >= 0.0)) return fail(TI_E_ARG, "weight_decay must be finite and >= 0");
    if (std::isnan(t.max_grad_norm)) return fail(TI_E_ARG, "max_grad_norm is NaN");
    return TI_OK;
}

struct Optim {
    AdamDesc td{};
    size_t nW = 0;
    long long n_applied = 0, n_skipped = 0;     // host mirror of ctr, read back at the end of every call that steps
    DevBuf<double> w, m, v, grad, sq, red, part64, log, bias;
    DevBuf<float> w32;
    DevBuf<long long> ctr;
    DevBuf<unsigned char> is_bias;              // [nW] 1 where the gradient is written in fp64 directly, not combined from slices
    std::vector<double> bias_tab;               // host side of bias: it outlives the copy that upload_bias enqueues

    // the state of a new trainer: the weights as given, zero moments, gradient and counters, the fp32 working copy.  n_red, n_log:
    // the entries of red and log a trainer wants from the start (n_log 0: none; a many-step call grows log).  The buffers are
    // allocated in the order either trainer allocated them before this header existed, so that their addresses stay where they were.
    void setup(const AdamDesc& t, const double* weights, const std::vector<unsigned char>& mask, size_t n_red, size_t n_log, hipStream_t st)
    {
        td = t; nW = mask.size();
        w.alloc(nW); m.alloc(nW); v.alloc(nW); grad.alloc(nW); sq.alloc(nW); w32.alloc(nW);
        red.alloc(n_red); ctr.alloc(2); log.alloc(n_log);
        is_bias.upload(mask);
        HIP_CHECK(hipMemcpyAsync(w.p, weights, nW * sizeof(double), hipMemcpyHostToDevice, st));
        for (DevBuf<double>* b : {&m, &v, &grad}) HIP_CHECK(hipMemsetAsync(b->p, 0, nW * sizeof(double), st));
        HIP_CHECK(hipMemsetAsync(ctr.p, 0, 2 * sizeof(long long), st));
        HIP_CHECK(launch_train_refresh(w32.p, w.p, nW, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }

    // the two bias terms of steps n_applied + 1 .. n_applied + n, computed here and indexed on the device by the steps applied so far
    void upload_bias(long long n, hipStream_t st)
    {
        bias_tab.resize(2 * (size_t)n);
        for (long long i = 0; i < n; ++i) {
            const double k = (double)(n_applied + 1 + i);
            bias_tab[2 * i] = td.lr / (1.0 - std::pow(td.beta1, k));
            bias_tab[2 * i + 1] = std::sqrt(1.0 - std::pow(td.beta2, k));
        }
        grow(bias, bias_tab.size());
        HIP_CHECK(hipMemcpyAsync(bias.p, bias_tab.data(), bias_tab.size() * sizeof(double), hipMemcpyHostToDevice, st));
    }

    // divisor: the entries the loss sum is a mean over (adw: B, painn: B A)
    TrAdam adam_params(bool with_loss, double divisor, double* log_out)
    {
        TrAdam a{};
        a.w = w.p; a.m = m.p; a.v = v.p; a.w32 = w32.p; a.grad = grad.p; a.n = nW;
        a.sumsq = red.p + RED_SUMSQ; a.loss_sum = with_loss ? red.p + RED_LOSS : nullptr; a.B = divisor;
        a.beta1 = td.beta1; a.beta2 = td.beta2; a.eps = td.eps; a.weight_decay = td.weight_decay; a.max_norm = td.max_grad_norm;
        a.bias = bias.p; a.ctr = ctr.p; a.base = n_applied; a.base_skip = n_skipped; a.log = log_out;
        return a;
    }

    void read_counters(hipStream_t st)
    {
        long long c[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        n_applied = c[0]; n_skipped = c[1];
    }

    void write_counters(hipStream_t st)
    {
        const long long c[2] = {n_applied, n_skipped};
        HIP_CHECK(hipMemcpyAsync(ctr.p, c, sizeof(c), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }

    // ti_*_train_apply: clip + Adam with the given gradient.  n_embed: launch_train_combine's (adw: its embedding entries, painn: 0)
    int apply(const double* g, int32_t* out_skipped, size_t n_embed, hipStream_t st)
    {
        grow(part64, (size_t)vloss_tiles((long long)nW));
        HIP_CHECK(hipMemcpyAsync(grad.p, g, nW * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_CHECK(launch_train_combine(grad.p, sq.p, nullptr, is_bias.p, 0, nW, n_embed, 0, 0, st));
        HIP_CHECK(launch_vloss_colsum(red.p + RED_SUMSQ, part64.p, sq.p, (long long)nW, 1, st));
        read_counters(st);                    // a call that failed half-way may have left the host mirror behind the device
        upload_bias(1, st);
        const TrAdam a = adam_params(false, 1.0, nullptr);
        HIP_CHECK(launch_train_adam(a, st));
        HIP_CHECK(launch_train_finish(a, st));
        const long long before = n_skipped;
        read_counters(st);
        if (out_skipped) *out_skipped = (int32_t)(n_skipped - before);
        return TI_OK;
    }

    int get_state(double* wo, double* mo, double* vo, int64_t* applied, int64_t* skipped, hipStream_t st)
    {
        const size_t bytes = nW * sizeof(double);
        if (wo) HIP_CHECK(hipMemcpyAsync(wo, w.p, bytes, hipMemcpyDeviceToHost, st));
        if (mo) HIP_CHECK(hipMemcpyAsync(mo, m.p, bytes, hipMemcpyDeviceToHost, st));
        if (vo) HIP_CHECK(hipMemcpyAsync(vo, v.p, bytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (applied) *applied = n_applied;
        if (skipped) *skipped = n_skipped;
        return TI_OK;
    }

    int set_state(const double* wi, const double* mi, const double* vi, int64_t applied, hipStream_t st)
    {
        const size_t bytes = nW * sizeof(double);
        if (wi) HIP_CHECK(hipMemcpyAsync(w.p, wi, bytes, hipMemcpyHostToDevice, st));
        if (mi) HIP_CHECK(hipMemcpyAsync(m.p, mi, bytes, hipMemcpyHostToDevice, st));
        if (vi) HIP_CHECK(hipMemcpyAsync(v.p, vi, bytes, hipMemcpyHostToDevice, st));
        if (wi) HIP_CHECK(launch_train_refresh(w32.p, w.p, nW, st));
        n_applied = applied;
        write_counters(st);
        return TI_OK;
    }

    // the tail of ti_*_train_grad: the loss rows (where mem says), the gradient and the two sums of the pass that has just been enqueued
    int grad_readback(double* out_loss, double* out_mean, double* out_grad, double* out_gnorm, long long B, double divisor, int mem,
                      const double* loss_buf, hipStream_t st)
    {
        double r[2];
        HIP_CHECK(hipMemcpyAsync(r, red.p, sizeof(r), hipMemcpyDeviceToHost, st));
        if (out_loss) HIP_CHECK(hipMemcpyAsync(out_loss, loss_buf, (size_t)B * sizeof(double), mem == TI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
        if (out_grad) HIP_CHECK(hipMemcpyAsync(out_grad, grad.p, nW * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (out_mean) *out_mean = r[RED_LOSS] / divisor;
        if (out_gnorm) *out_gnorm = std::sqrt(r[RED_SUMSQ]);
        return TI_OK;
    }

    // the tail of a many-step call: the logged losses, the counters (the call's synchronisation), the steps it skipped
    void steps_readback(double* out_loss, int64_t* out_skipped, int64_t n_steps, hipStream_t st)
    {
        if (out_loss) HIP_CHECK(hipMemcpyAsync(out_loss, log.p, (size_t)n_steps * sizeof(double), hipMemcpyDeviceToHost, st));
        const long long before = n_skipped;
        read_counters(st);
        if (out_skipped) *out_skipped = n_skipped - before;
    }
};

// ---- the indices [n_idx] of a many-step call into sets of n0 and n1 rows, where mem says (check0 false: set 0 is not read, idx0 is
// not checked).  Host indices are checked ahead of the handle check; device indices are read back once and checked inside the call,
// before anything is enqueued.  Either way the kernels read them through Staged::in.
static_assert(sizeof(long long) == sizeof(int64_t), "index width");
inline const long long* idx_ll(const int64_t* p) { return reinterpret_cast<const long long*>(p); }

inline int train_idx_check(const int64_t* i0, const int64_t* i1, size_t n_idx, int64_t n0, int64_t n1, bool check0, int mem)
{
    std::vector<int64_t> h0, h1;
    if (mem != TI_MEM_HOST) {
        h0.resize(n_idx); h1.resize(n_idx);
        HIP_CHECK(hipMemcpy(h0.data(), i0, n_idx * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(h1.data(), i1, n_idx * sizeof(int64_t), hipMemcpyDeviceToHost));
        i0 = h0.data(); i1 = h1.data();
    }
    for (size_t k = 0; k < n_idx; ++k) {
        if (check0 && (i0[k] < 0 || i0[k] >= n0)) return fail(TI_E_ARG, "idx0[" + std::to_string(k) + "] is outside 0..n0-1");
        if (i1[k] < 0 || i1[k] >= n1) return fail(TI_E_ARG, "idx1[" + std::to_string(k) + "] is outside 0..n1-1");
    }
    return TI_OK;
}

}  // namespace
}  // namespace ti
