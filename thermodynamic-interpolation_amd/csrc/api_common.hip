// api_common.hip -- what every handle kind shares of the C ABI (include/ti_hip.h): version, the per-thread error text, workspace
// reservation, stream binding, live kernel timing with HIP events, destruction, and the device self-test.
#include "ti_handle.hpp"

namespace ti {

static thread_local std::string g_err;      // the one error text of the library: every unit fails through fail()
int fail(int code, const std::string& msg) { g_err = msg; return code; }

}  // namespace ti

extern "C" {

int ti_version(void) { return TI_ABI_VERSION; }

int ti_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

const char* ti_last_error(void) { return g_err.c_str(); }

int64_t ti_rollout_rows(int32_t n_step, int32_t save_every)
{
    if (save_every <= 0) return 1;
    const int64_t steps = n_step - 1;
    return steps / save_every + 1 + (steps % save_every != 0);
}

int ti_reserve(ti_handle* h, int64_t B)
{
    if (!h || B < 0) return fail(TI_E_ARG, "bad handle / B");
    if (h->kind >= 2) return fail(TI_E_ARG, "a trainer handle sizes its workspace per call: ti_reserve takes painn and adw handles");
    return guarded([&]() -> int { set_device(h); if (h->kind == 0) ensure_painn_ws(h, B); else ensure_adw_ws(h, B); return TI_OK; });
}

int ti_rollout_step_counts(ti_handle* h, int64_t* accepted, int64_t* rejected, int64_t B)
{
    if (!h || !accepted || !rejected) return fail(TI_E_ARG, "NULL argument");
    if (B != (int64_t)h->traj_accepted.size())
        return fail(TI_E_ARG, "B = " + std::to_string(B) + " does not match the last per-trajectory rollout (" + std::to_string(h->traj_accepted.size()) + " trajectories)");
    std::copy(h->traj_accepted.begin(), h->traj_accepted.end(), accepted);
    std::copy(h->traj_rejected.begin(), h->traj_rejected.end(), rejected);
    return TI_OK;
}

void ti_destroy(ti_handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

int ti_set_stream(ti_handle* h, void* hip_stream, int mode)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    if (mode != TI_STREAM_OWN && mode != TI_STREAM_EXTERNAL) return fail(TI_E_ARG, "unknown stream mode");
    h->stream = mode == TI_STREAM_EXTERNAL ? reinterpret_cast<hipStream_t>(hip_stream) : h->own_stream;
    return TI_OK;
}

int ti_wait_stream(ti_handle* h, void* producer_stream)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t prod = reinterpret_cast<hipStream_t>(producer_stream);
        if (prod == h->stream) return TI_OK;                     // same stream: already ordered
        if (!h->wait_ev) HIP_CHECK(hipEventCreateWithFlags(&h->wait_ev, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(h->wait_ev, prod));
        HIP_CHECK(hipStreamWaitEvent(h->stream, h->wait_ev, 0));
        return TI_OK;
    });
}

int ti_profile_enable(ti_handle* h, int on)
{
    if (!h) return fail(TI_E_ARG, "NULL handle");
    h->prof = on != 0;
    return TI_OK;
}

int ti_profile_read(ti_handle* h, int kernel, int64_t* n_launches, double* total_ms)
{
    if (!h || kernel < 0 || kernel >= TI_KERNEL_COUNT) return fail(TI_E_ARG, "bad handle / kernel id");
    return guarded([&]() -> int {
        set_device(h);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        double tot = 0; int64_t cnt = 0;
        for (auto& pr : h->ev[kernel]) {
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, pr.first, pr.second));
            tot += ms; ++cnt;
            (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second);
        }
        h->ev[kernel].clear();
        if (n_launches) *n_launches = cnt;
        if (total_ms) *total_ms = tot;
        return TI_OK;
    });
}

int ti_selftest(int device)
{
    return guarded([&]() -> int {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TI_E_HIP, "no HIP device");
        HIP_CHECK(hipSetDevice(device));
        DevBuf<float> d; d.alloc(64 * 16);
        HIP_CHECK(launch_selftest(d.p, nullptr));
        std::vector<float> o(64 * 16);
        HIP_CHECK(hipMemcpy(o.data(), d.p, o.size() * sizeof(float), hipMemcpyDeviceToHost));
        // expected D[i][j] = sum_k A[i][k] B[k][j], A[i][k] = 1 + i + 100k, B[k][j] = 1000 + j - 7k;
        // accumulator register r of lane l holds row (r&3) + 8*(r>>2) + 4*(l>>5), column l&31
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 16; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), j = l & 31;
                double ref = 0;
                for (int k = 0; k < 2; ++k) ref += (1.0 + i + 100.0 * k) * (1000.0 + j - 7.0 * k);
                if (std::fabs(o[l * 16 + r] - ref) > 1e-3 * std::fabs(ref))
                    return fail(TI_E_HIP, "MFMA 32x32x2 lane map differs from the layout the kernels assume (lane " + std::to_string(l) +
                                              ", reg " + std::to_string(r) + ")");
            }
        // the 8-instruction operand split (v_fma_mix lo/hi, half-register writes) against the plain arithmetic, 16.8 M values
        DevBuf<unsigned> cnt; cnt.alloc(2);
        HIP_CHECK(hipMemset(cnt.p, 0, 2 * sizeof(unsigned)));
        HIP_CHECK(launch_split_selftest(cnt.p, nullptr));
        unsigned bad[2] = {0, 0};
        HIP_CHECK(hipMemcpy(bad, cnt.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
        if (bad[0]) return fail(TI_E_HIP, "operand split: " + std::to_string(bad[0]) + " fp16 halves differ from the reference arithmetic (either format)");
        if (bad[1]) return fail(TI_E_HIP, "v_mfma_f32_16x16x32_f16 flushed fp16-subnormal inputs: the one-accumulator operand format needs them kept");
        return TI_OK;
    });
}

}  // extern "C"
