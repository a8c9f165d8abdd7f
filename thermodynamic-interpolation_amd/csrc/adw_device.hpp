// adw_device.hpp -- device code shared by the adw translation units (adw_kernels.hip, adw_fused_kernels.hip): the register-resident
// FCNetMultiBeta MLP body and the Philox normal of TI_SCHEME_EM.  One definition each, so the per-call drift kernel and the fused
// rollout kernel run the same source and the fused rollout can be bit-identical to the host-driven one.
#pragma once
#include "mfma_chain.hpp"

namespace ti {

// Linear(3 -> H), SiLU, [Linear(H -> H), SiLU] x n_hidden, Linear(H -> 1) on the rows (a0, a1, a2) of one wave (16 rows, lane = row j +
// 16 q): hidden activations stay in registers, H x H layers on the matrix cores from the weight ring `pipe` (one acquire / release per
// 32-output chunk, n_hidden * NB per evaluation -- a whole turn of the cyclic stream, so evaluations can follow each other).
// w_in [H][3] | b_in [H] | b_hid [n_hidden][H] | w_out [H] are LDS pointers.  o = the output; TAN: d = d o / d a0 (forward mode).
template <int NBK, bool SPLIT, bool TAN, typename Pipe>
__device__ __forceinline__ void adw_net_eval(Pipe& pipe, const float* w_in, const float* b_in, const float* b_hid, const float* w_out,
                                             int n_hidden, float b_out, float a0, float a1, float a2, int lane, int q, float& o, float& d)
{
    constexpr int H = 16 * NBK, NB = (H + 31) / 32;
    using A16 = r16::Act<NBK>;
    using OP = r16::Opnd<NBK, SPLIT>;
    // silu(z) = z * sig(z);  silu'(z) = sig(z) + silu(z) * (1 - sig(z))
    auto act = [](float z, float& y, float& dy) {
        const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-z));
        y = z * sg;
        dy = fmaf(y, 1.0f - sg, sg);
    };
    // input layer (K = 3): plain FMAs straight into the register layout
    A16 cur, tan;
#pragma unroll
    for (int nb = 0; nb < NBK; ++nb) {
        const float* w = w_in + (16 * nb + 4 * q) * 3;                     // rows f..f+3 of W_in[H][3]
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(w), w1 = *reinterpret_cast<const f32x4*>(w + 4),
                    w2 = *reinterpret_cast<const f32x4*>(w + 8);
        const float ww[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
        const f32x4 bb = r16::load_block(b_in, nb, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float z = fmaf(ww[3 * k + 2], a2, fmaf(ww[3 * k + 1], a1, fmaf(ww[3 * k], a0, bb[k])));
            float y, dy;
            act(z, y, dy);
            cur.b[nb][k] = y;
            if (TAN) tan.b[nb][k] = dy * ww[3 * k];
        }
    }
    // hidden layers
    for (int l = 0; l < n_hidden; ++l) {
        OP in, tin;
        in.set(cur);
        if (TAN) tin.set(tan);
        const float* bias = b_hid + (size_t)l * H;
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 z0 = r16::load_block(bias, 2 * ch, q), z1 = r16::load_block(bias, 2 * ch + 1, q);
            r16::gemm_bt(z0, z1, in, wl, lane);
            f32x4 t0 = {0, 0, 0, 0}, t1 = {0, 0, 0, 0};
            if (TAN) r16::gemm_bt(t0, t1, tin, wl, lane);
            pipe.release();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float y, dy;
                act(z0[k], y, dy); cur.b[2 * ch][k] = y;     if (TAN) tan.b[2 * ch][k] = dy * t0[k];
                act(z1[k], y, dy); cur.b[2 * ch + 1][k] = y; if (TAN) tan.b[2 * ch + 1][k] = dy * t1[k];
            }
        }
    }
    o = 0.f; d = 0.f;
#pragma unroll
    for (int nb = 0; nb < NBK; ++nb) {
        const f32x4 w = r16::load_block(w_out, nb, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) { o = fmaf(cur.b[nb][k], w[k], o); if (TAN) d = fmaf(tan.b[nb][k], w[k], d); }
    }
    o = r16::xquarters(o) + b_out;
    if (TAN) d = r16::xquarters(d);
}

// Philox4x32-10, same function as oracle/ti_oracle.c:ti_normal (build-defined, include/ti_hip.h TI_SCHEME_EM)
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ float ti_normal(uint64_t seed, long long traj, int step, int comp)
{
    uint32_t c[4] = {(uint32_t)traj, (uint32_t)((uint64_t)traj >> 32), (uint32_t)step, (uint32_t)(comp >> 2)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int pair = (comp & 3) >> 1;
    const float u1 = ((float)(c[2 * pair] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2 * pair + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1)), a = 6.283185307179586f * u2;
    return (comp & 1) ? r * sinf(a) : r * cosf(a);
}

}  // namespace ti
