// adw_fused_kernels.hip -- a whole fixed-step adw rollout (Euler / Heun / Euler-Maruyama, 1-D handles) in one kernel launch.
//
// The host-driven rollout (rollout.hpp: rollout_common) launches per step the beta embedding, `net`, one or two update kernels and for EM
// the noise kernel; x and b travel through HBM between them.  The particles are independent and the weights already stream through a
// cyclic LDS ring, so nothing in the arithmetic needs the host between steps: here a wave keeps its 16 particles (x, and the dlogp
// state with TAN) in registers for all n_step - 1 steps, evaluates `net` through the SAME device function as adw_mlp_kernel
// (adw_device.hpp: adw_net_eval), applies the updates of axpy_kernel / heun_kernel / noise_kernel / scale_kernel, and writes only the
// saved rows.  Those kernels spell `x + a * b` with __fadd_rn / __fmul_rn, which HIP defines as the plain operators: hipcc contracts
// each of them to ONE v_fmac_f32 (adw_kernels.hip's disassembly), so the update the unfused rollout actually computes is fma(a, b, x).
// Here that is written as an explicit fmaf, so that no context-dependent choice of the compiler stands between the two paths.
// Per-step scalars come from a host-filled table, the beta embedding from a table the existing embedding kernel filled in one
// launch: the kernel computes neither.  Bit-identical to the host-driven rollout.
#include "adw_device.hpp"
#include "mfma_chain.hpp"
#include "ti_internal.hpp"

namespace ti {

// Workgroup shape of adw_mlp_kernel: 4 waves, 16 rows per wave, grid ceil(B / 64), PipeDMA<NB, T, 1> over the `net` stream.  Every
// wave -- those whose rows all lie beyond B included (clamped row, `ok`) -- makes the same n_hidden * NB acquire / release trips per
// evaluation, so the ring's barriers stay uniform; Heun is a uniform run-time branch (p.scheme is a kernel argument).
template <int NBK, bool SPLIT, bool TAN>
__global__ __launch_bounds__(256, (NBK <= 8 && !TAN) ? 2 : 1) void adw_rollout_fused_kernel(const AdwFusedParams p)
{
    constexpr int H = 16 * NBK, NB = (H + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = 256 * NB;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    float* vec = reinterpret_cast<float*>(lds + 2 * CH4);
    const int nvec4 = (5 + p.n_hidden) * H / 4;
    for (int i = threadIdx.x; i < nvec4; i += T) reinterpret_cast<f32x4*>(vec)[i] = reinterpret_cast<const f32x4*>(p.vecs)[i];
    PipeDMA<NB, T, 1> pipe;
    if (p.nch > 0) pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);
    else __syncthreads();
    const float* w_in = vec;
    const float* b_in = vec + 3 * H;
    const float* b_hid = vec + 4 * H;
    const float* w_out = vec + (4 + p.n_hidden) * H;

    const long long row = ((long long)blockIdx.x * WAVES + wave) * 16 + j;
    const bool ok = row < p.B, wr = ok && q == 0;
    const long long r = ok ? row : p.B - 1;
    const float* emb = p.emb + p.idx[r];             // emb[k * U + idx[row]]
    float x = p.x[r], dl = 0.f;
    long long orow = 0;                              // next row of out_path / out_dlogp
    auto save = [&]() {
        if (wr) {
            p.out_path[orow * p.B + row] = x;
            if (TAN) p.out_dlogp[orow * p.B + row] = dl * p.out_scale;       // scale_kernel's single multiply
        }
        ++orow;
    };
    if (p.save_every > 0) save();
    const int nstage = p.scheme == ADW_FUSED_HEUN ? 2 : 1;
    for (int k = 0; k < p.n_step - 1; ++k) {
        const AdwFusedStep s = p.steps[k];
        float b1 = 0.f, d1 = 0.f, b2 = 0.f, d2 = 0.f;
        for (int stage = 0; stage < nstage; ++stage) {
            // Heun's second drift: at t_{k+1} on x + dt b1 (axpy_kernel), held in registers
            const float xin = stage ? fmaf(s.dt, b1, x) : x;
            const float tin = stage ? s.t_next : s.t;
            const float ein = emb[(size_t)(k + stage) * p.U];
            float o, d;
            adw_net_eval<NBK, SPLIT, TAN>(pipe, w_in, b_in, b_hid, w_out, p.n_hidden, p.b_out, xin, tin, ein, lane, q, o, d);
            if (stage) { b2 = o; d2 = d; } else { b1 = o; d1 = d; }
        }
        if (nstage == 2) {                           // heun_kernel
            x = fmaf(s.hdt, b1 + b2, x);
            if (TAN) dl = fmaf(s.nhdt, d1 + d2, dl);
        } else {                                     // axpy_kernel, then noise_kernel at comps = 1 without centre-of-mass removal
            x = fmaf(s.dt, b1, x);
            if (TAN) dl = fmaf(s.ndt, d1, dl);
            if (p.scheme == ADW_FUSED_EM) x = fmaf(s.sigma, ti_normal(p.seed, p.traj0 + r, p.step0 + k, 0), x);
        }
        const int step = k + 1;
        if (p.save_every > 0 && (step % p.save_every == 0 || step == p.n_step - 1)) save();
    }
    if (p.save_every <= 0) save();
    if (wr) p.x[row] = x;                            // the end state stays in the handle for the non-finite check
    pipe.drain();
}

static size_t adw_fused_lds_bytes(int NB, int n_hidden) { return 2 * (size_t)256 * NB * 16 + (size_t)(5 + n_hidden) * 32 * NB * 4; }

// 16 instantiations: H in {32, 64, 128, 256} x {f32, f16x2} x {drift only, with tangent}
#define TI_FUSED_DISPATCH_NB(NBv, ...) \
    switch (NBv) {                                                            \
        case 1: { constexpr int NB = 1; __VA_ARGS__; } break;                 \
        case 2: { constexpr int NB = 2; __VA_ARGS__; } break;                 \
        case 4: { constexpr int NB = 4; __VA_ARGS__; } break;                 \
        case 8: { constexpr int NB = 8; __VA_ARGS__; } break;                 \
        default: return hipErrorInvalidValue;                                 \
    }

template <int NBK>
static hipError_t adw_fused_set_attrs(size_t bytes)
{
    hipError_t e;
#define TI_SET(k) if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) != hipSuccess) return e
    TI_SET((adw_rollout_fused_kernel<NBK, false, false>)); TI_SET((adw_rollout_fused_kernel<NBK, true, false>));
    TI_SET((adw_rollout_fused_kernel<NBK, false, true>)); TI_SET((adw_rollout_fused_kernel<NBK, true, true>));
#undef TI_SET
    return hipSuccess;
}

hipError_t configure_adw_fused_kernels(int NBv, int max_hidden)
{
    TI_FUSED_DISPATCH_NB(NBv, return (adw_fused_set_attrs<2 * NB>(adw_fused_lds_bytes(NB, max_hidden))));
    return hipSuccess;
}

hipError_t launch_adw_fused(int NBv, bool split, const AdwFusedParams& p, hipStream_t st)
{
    if (p.B <= 0) return hipSuccess;
    TI_FUSED_DISPATCH_NB(NBv, {
        const dim3 g((unsigned)((p.B + 63) / 64));
        const size_t l = adw_fused_lds_bytes(NB, p.n_hidden);
        const bool tanv = p.out_dlogp != nullptr;
        if (split) {
            if (tanv) hipLaunchKernelGGL((adw_rollout_fused_kernel<2 * NB, true, true>), g, dim3(256), l, st, p);
            else hipLaunchKernelGGL((adw_rollout_fused_kernel<2 * NB, true, false>), g, dim3(256), l, st, p);
        } else {
            if (tanv) hipLaunchKernelGGL((adw_rollout_fused_kernel<2 * NB, false, true>), g, dim3(256), l, st, p);
            else hipLaunchKernelGGL((adw_rollout_fused_kernel<2 * NB, false, false>), g, dim3(256), l, st, p);
        }
    });
    return hipGetLastError();
}

}  // namespace ti
