// painn_jvp_kernels.hip -- forward-mode derivative of the cPaiNN drift for gfx950 (MI355X): the exact divergence the
// reference obtains with 3A reverse-mode passes (ODEWrapper.compute_divergence,
// /root/reference/mdqm9/thermo/ambient/models/ode_wrapper.py:59-91; latent twin ode_wrapper.py:57-86).
//
// Virtual molecules.  Molecule b differentiated along seed direction d is a "virtual molecule".  D = 3A with unit seeds
// (d perturbs atom d / 3, component d % 3) gives the Jacobian diagonal, D = 1 with an explicit xdot an arbitrary JVP.
// They are grouped like the primal molecules: primal group pg (G molecules, one wave) and direction d form virtual group
// vg = pg * D + d, whose G members are the G molecules of pg -- so virtual row (blk, j) IS primal row (blk, j) of group pg
// (with P > 1 parts per group, ti_internal.hpp, every part of every direction has its own wave: gi = (pg * D + d) * P + part)
// (same edge, same slot), and the D directions of one primal group are neighbours in the launch (their primal reads hit L2).
//   virtual molecule vm = vg * G + m  <->  molecule pm = pg * G + m;   virtual node = vm * A + atom.
// The kernels carry ONLY tangents in HBM (ts, tv, te, tP and three accumulators, laid out like their primal twins over
// virtual molecules).  Primal state is read from the ordinary drift pipeline, which the host runs in lock step
// (painn_host.hip: [filter pass ->] tangent edge -> primal edge -> tangent update -> primal update per layer); the primal
// activations a tangent needs (LayerNorm statistics, SiLU slopes, gate values) are recomputed in registers next to it, every
// matrix product runs on a (value, tangent) operand pair against one weight chunk in LDS.
//
// The filter branch w(enc(|r|)) depends on x only through the edge length, so its tangent is rank one:
//   d w_o[edge][dir] = d|r|[edge][dir] * Q[edge],  Q = (d w_o / d |r|).
// painn_jvp_filter_kernel (the "primal pass") evaluates w_o and Q ONCE per primal edge and layer (a dual pass seeded with
// d|r| = 1), together with the phi branch's forward values and LayerNorm statistics, and parks them in HBM in the register
// layouts the per-direction edge kernel consumes; that kernel is left with the TANGENT of the phi branch only -- a quarter
// of the matrix work of differentiating both branches per direction, and no transcendental per (edge, direction).
//
// Tangent rules restated from the forward pass (painn_kernels.hip; reference lines there):
//   geometry  r = x_s - x_d, d = |r|, dir = r / (1 + d):   dd = r.dr / d,  ddir = dr / (1 + d) - r dd / (1 + d)^2
//   products  (h g)' = h' g + h g' ;  cross(k, v)' = cross(k', v) + cross(k, v')
//   norm      n = |V v|:  n' = (V v).(V v') / n   (0 at n = 0, like torch.norm's backward)
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "dispatch.hpp"
#include "mfma_chain.hpp"
#include "ti_internal.hpp"

namespace ti {

namespace {

struct EV {          // same vector block as painn_kernels.hip (struct EV)
    static constexpr int W_B0 = 0, W_G0 = 1, W_BE0 = 2, W_B1 = 3, W_G1 = 4, W_BE1 = 5, P_G0 = 6, P_BE0 = 7, P_B1 = 8, P_G1 = 9,
                         P_BE1 = 10, P_B2 = 11, W_B2 = 16, COUNT = 21;
};
struct UV {          // same vector block as painn_kernels.hip (struct UV)
    static constexpr int B0 = 0, G0 = 1, BE0 = 2, B1 = 3, G1 = 4, BE1 = 5, B2 = 6, PB0 = 9, COUNT = 10;
};
struct RV {          // readout vector block: b0 g0 be0 b1 g1 be1 w2_gate Vr
    static constexpr int B0 = 0, G0 = 1, BE0 = 2, B1 = 3, G1 = 4, BE1 = 5, W2G = 6, VR = 7, COUNT = 8;
};

__device__ __forceinline__ void add_noret(float* p, float v) { unsafeAtomicAdd(p, v); }
// accumulator update with the first-touch rule of the primal edge kernel (ti_internal.hpp SLOT_FIRST_TOUCH)
__device__ __forceinline__ void acc_out(float* p, float v, bool first)
{
    if (first) (void)__hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else unsafeAtomicAdd(p, v);
}

#define Z4 (f32x4{0.f, 0.f, 0.f, 0.f})

}  // namespace

// ================================================================================================== primal pass
// Everything the per-direction edge kernel needs from the forward pass of this layer's message block, ONCE per primal edge:
//   wq[((((pg * nblk + blk) * 5 + c) * NB + nbo) * 6 + k) * 64 + lane]  (float4 = the block's rows 4 (lane >> 4) .. + 3)
//        k = 0/1: phi_o + bias (features 32 nbo + {0,16} + (lane & 15)),  2/3: w_o + bias,  4/5: Q = d w_o / d|r|
//   st[(((pg * nblk + blk) * 4 + which) * NBK + nb) * 64 + lane]        which = n, kk of phi's two LayerNorms (ln_silu_stats),
//        float4 = features 16 nb + 4 (lane >> 4) .. + 3 of row (lane & 15)
// The filter branch runs as a (value, tangent) pair seeded with d|r| = 1 (-> Q), the phi branch as the plain forward pass.
// Reads the primal edge stream of painn_edge_kernel (same chunk order); one wave per primal group.
template <int NBK, bool SPLIT>
__global__ __launch_bounds__(256, 1) void painn_jvp_filter_kernel(const JvpFilterParams p)
#define TI_FILTER_ROWS_GROUP gi - mg * p.parts
#include "painn_jvp_filter_body.inc"
#undef TI_FILTER_ROWS_GROUP

// Per-molecule edge types (ti_painn_set_molecules): p.rows holds row words per (group, part) (painn_pack.hip: masked_rows), whose type bits
// are each molecule's own.  The filter pass reads nothing else from them that a mask changes (it ignores slots).
template <int NBK, bool SPLIT>
__global__ __launch_bounds__(256, 1) void painn_jvp_filter_mask_kernel(const JvpFilterParams p)
#define TI_FILTER_ROWS_GROUP gi
#include "painn_jvp_filter_body.inc"
#undef TI_FILTER_ROWS_GROUP

// ================================================================================================== tangent edge kernel
// One wave per virtual group.  Per (edge, direction) row only TANGENT products remain: the phi branch's hidden layers and
// output chunks applied to the tangent of [s[src] | e]; every primal quantity comes from the primal pass above.
template <int NBK, bool SPLIT>
__global__ __launch_bounds__(256, (NBK <= 8 ? 2 : 1)) void painn_jvp_edge_kernel(const JvpEdgeParams p)
#define TI_ROWS_GROUP part
#include "painn_jvp_edge_body.inc"
#undef TI_ROWS_GROUP

// Per-molecule edge sets (ti_painn_set_edge_mask): p.rows holds row words per PRIMAL (group, part) (painn_pack.hip: masked_rows), in which
// a template row whose edge is absent from its molecule has slot 63: weight 0 in the tangent sums, like a padding row.  First-touch
// writes are the template's.  An all-ones mask gives painn_jvp_edge_kernel's bits.
template <int NBK, bool SPLIT>
__global__ __launch_bounds__(256, (NBK <= 8 ? 2 : 1)) void painn_jvp_edge_mask_kernel(const JvpEdgeParams p)
#define TI_ROWS_GROUP (int)pg
#include "painn_jvp_edge_body.inc"
#undef TI_ROWS_GROUP

// ================================================================================================== primal node pass
// Everything the per-direction update kernel needs from the forward pass of this layer's update block, ONCE per primal node
// (16 nodes per wave, chain layout: float4 = features 16 nb + 4 (lane >> 4) .. + 3 of node row (lane & 15)):
//   ns[((tile * NS_COUNT + which) * NBK + nb) * 64 + lane],  tile = node / 16,  which:
//     0..2 vv_c / |vv|   (c = x, y, z; vv = V v_eff; 0 where |vv| = 0 like torch.norm's backward)
//     3    |vv|          4..7 n, kk of the update MLP's two LayerNorms      8 scale_squared_norm output   9 gates
//     10..12 U v_eff
// Runs after the primal edge kernel and before the primal update kernel of the layer (reads what the latter overwrites).
constexpr int NS_COUNT = 13;
template <int NBK, bool SPLIT>
__global__ __launch_bounds__(256, 1) void painn_jvp_node_kernel(const JvpNodeParams p)
{
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = 256 * NB;
    using A16 = r16::Act<NBK>;
    using OP = r16::Opnd<NBK, SPLIT>;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    float* vec = reinterpret_cast<float*>(lds + 4 * CH4);
    for (int i = threadIdx.x; i < UV::COUNT * F / 4; i += T)
        reinterpret_cast<f32x4*>(vec)[i] = reinterpret_cast<const f32x4*>(p.vecs)[i];
    PipeDMA<NB, T, 2> pipe;
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);

    const long long tile = (long long)blockIdx.x * WAVES + wave;
    const long long node = tile * 16 + j;
    const bool tile_ok = tile * 16 < p.N;
    const size_t pn = (size_t)(node < p.N ? node : p.N - 1);
    const float *vb = p.v + pn * 3 * F, *db = p.dvacc + pn * 3 * F, *cb = p.cacc + pn * 3 * F, *sb = p.s + pn * F, *ab = p.dsacc + pn * F;
    f32x4* nsp = reinterpret_cast<f32x4*>(p.ns) + ((size_t)(tile_ok ? tile : 0) * NS_COUNT * NBK) * 64 + lane;
    auto park = [&](int which, const A16& v) {
        if (tile_ok) {
#pragma unroll
            for (int nb = 0; nb < NBK; ++nb) nsp[(size_t)(which * NBK + nb) * 64] = v.b[nb];
        }
    };
    auto veff = [&](int c, A16& t) {
        const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) {
            const f32x4 vc = r16::load_block(vb + c * F, nb, q), dd = r16::load_block(db + c * F, nb, q);
            const f32x4 v1 = r16::load_block(vb + c1 * F, nb, q), v2 = r16::load_block(vb + c2 * F, nb, q);
            const f32x4 k1 = r16::load_block(cb + c1 * F, nb, q), k2 = r16::load_block(cb + c2 * F, nb, q);
            t.b[nb] = (vc + dd) + (k1 * v2 - k2 * v1);
        }
    };
    // ---- phase A: vv_c = V v_eff_c (parked raw, normalised at the end of the phase), n2 = |vv|^2
    A16 n2;
#pragma unroll
    for (int nb = 0; nb < NBK; ++nb) n2.b[nb] = Z4;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        OP ve;
        float vsc;                                  // v is an un-normalised stream
        {
            A16 t;
            veff(c, t);
            vsc = ve.set_scaled(t);
        }
        A16 vv;
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = Z4, a1 = Z4;
            r16::gemm_bt_sc(a0, a1, ve, vsc, wl, lane);
            vv.b[2 * ch] = a0; vv.b[2 * ch + 1] = a1;
            n2.b[2 * ch] += a0 * a0; n2.b[2 * ch + 1] += a1 * a1;
            pipe.release();
        }
        park(c, vv);
    }
#pragma unroll
    for (int nb = 0; nb < NBK; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) n2.b[nb][r] = sqrtf(n2.b[nb][r]);
    park(3, n2);
    if (tile_ok) {                                 // vv_c <- vv_c / |vv| in place (same lane wrote it)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int nb = 0; nb < NBK; ++nb) {
                f32x4 v = nsp[(size_t)(c * NBK + nb) * 64];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = n2.b[nb][r] > 0.f ? v[r] / n2.b[nb][r] : 0.f;
                nsp[(size_t)(c * NBK + nb) * 64] = v;
            }
    }
    // ---- phase B: MLP([ |vv| , s + ds ]) with parked LayerNorm statistics
    OP h2;
    {
        A16 t;
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) t.b[nb] = r16::load_block(vec + UV::B0 * F, nb, q);
        {
            OP nn;
            const float nsc = nn.set_scaled(n2);
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                r16::gemm_bt_sc(t.b[2 * ch], t.b[2 * ch + 1], nn, nsc, wl, lane);
                pipe.release();
            }
        }
        {
            OP ss;
            float ssc;
            {
                A16 x;
#pragma unroll
                for (int nb = 0; nb < NBK; ++nb) x.b[nb] = r16::load_block(sb, nb, q) + r16::load_block(ab, nb, q);
                ssc = ss.set_scaled(x);
            }
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                r16::gemm_bt_sc(t.b[2 * ch], t.b[2 * ch + 1], ss, ssc, wl, lane);
                pipe.release();
            }
        }
        {
            A16 nn, kk;
            r16::ln_silu_stats(t, nn, kk, vec + UV::G0 * F, vec + UV::BE0 * F, q);
            park(4, nn); park(5, kk);
        }
        {
            OP h1;
            h1.set(t);
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                f32x4 a0 = r16::load_block(vec + UV::B1 * F, 2 * ch, q), a1 = r16::load_block(vec + UV::B1 * F, 2 * ch + 1, q);
                r16::gemm_bt(a0, a1, h1, wl, lane);
                t.b[2 * ch] = a0; t.b[2 * ch + 1] = a1;
                pipe.release();
            }
        }
        {
            A16 nn, kk;
            r16::ln_silu_stats(t, nn, kk, vec + UV::G1 * F, vec + UV::BE1 * F, q);
            park(6, nn); park(7, kk);
        }
        h2.set(t);
    }
    {   // scale_squared_norm (the add_invariant chunk is skipped: it enters no tangent), then gates
        A16 qq, gg;
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 q0 = r16::load_block(vec + (UV::B2 + 1) * F, 2 * ch, q), q1 = r16::load_block(vec + (UV::B2 + 1) * F, 2 * ch + 1, q);
            r16::gemm_bt(q0, q1, h2, wl, lane);
            qq.b[2 * ch] = q0; qq.b[2 * ch + 1] = q1;
            pipe.release();
            (void)pipe.acquire();
            pipe.release();
        }
        park(8, qq);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = r16::load_block(vec + UV::B2 * F, 2 * ch, q), a1 = r16::load_block(vec + UV::B2 * F, 2 * ch + 1, q);
            r16::gemm_bt(a0, a1, h2, wl, lane);
            gg.b[2 * ch] = a0; gg.b[2 * ch + 1] = a1;
            pipe.release();
        }
        park(9, gg);
    }
    // ---- phase C: U v_eff
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        OP ve;
        float vsc;
        {
            A16 t;
            veff(c, t);
            vsc = ve.set_scaled(t);
        }
        A16 uv;
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = Z4, a1 = Z4;
            r16::gemm_bt_sc(a0, a1, ve, vsc, wl, lane);
            uv.b[2 * ch] = a0; uv.b[2 * ch + 1] = a1;
            pipe.release();
        }
        park(10 + c, uv);
    }
    pipe.drain();
}

// ================================================================================================== tangent update kernel
// Runs BEFORE the primal update kernel of the same layer: reads the primal v and cacc as the edge kernel left them and the
// primal node pass output, advances ts, tv, tP; the tangent accumulators are consumed and zeroed.  Tangent products only.
template <int NBK, bool SPLIT>
__global__ __launch_bounds__(256, (NBK <= 8 ? 2 : 1)) void painn_jvp_update_kernel(const JvpUpdateParams p)
{
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = 256 * NB;
    using A16 = r16::Act<NBK>;
    using OP = r16::Opnd<NBK, SPLIT>;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    PipeDMA<NB, T, 2> pipe;
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);

    const long long node = ((long long)blockIdx.x * WAVES + wave) * 16 + j;      // virtual node
    const long long nd = node < p.N ? node : p.N - 1;
    const long long vm = nd / p.A, vg = vm / p.G;
    const long long pm_raw = (vg / p.D) * p.G + (vm - vg * p.G);                      // molecule of this virtual molecule
    const bool ok = node < p.N && pm_raw < p.B;
    const size_t pn = (size_t)((pm_raw < p.B ? pm_raw : p.B - 1) * p.A + (nd - vm * p.A));   // primal node
    const float *vb = p.v + pn * 3 * F, *cb = p.cacc + pn * 3 * F;
    float *tvb = p.tv + (size_t)nd * 3 * F, *tdb = p.tdvacc + (size_t)nd * 3 * F, *tcb = p.tcacc + (size_t)nd * 3 * F;
    float *tsb = p.ts + (size_t)nd * F, *tab = p.tdsacc + (size_t)nd * F;
    // node-pass data of THIS lane's primal node: tile pn / 16, row pn % 16, this lane's feature quarter q
    const f32x4* nsp = reinterpret_cast<const f32x4*>(p.ns) + ((pn >> 4) * NS_COUNT * NBK) * 64 + (q * 16 + (pn & 15));
    auto stat = [&](int which, int nb) { return nsp[(size_t)(which * NBK + nb) * 64]; };

    // ---- phase A: tv_eff (parked in tdvacc), n' = sum_c (vv_c / |vv|) . (V tv_eff_c)
    // Feature block outermost, like the primal update kernel: tv, tcacc and tdvacc are read once each (the cross product needs all three
    // components of a block; per-component loops read tv three times and tcacc twice, and those repeats came from HBM).
    A16 tn;
#pragma unroll
    for (int nb = 0; nb < NBK; ++nb) tn.b[nb] = Z4;
    {
        A16 u[3];
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) {
            f32x4 vv[3], kk[3], tvv[3], tkk[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                vv[c] = r16::load_block(vb + c * F, nb, q); kk[c] = r16::load_block(cb + c * F, nb, q);
                tvv[c] = r16::load_block(tvb + c * F, nb, q); tkk[c] = r16::load_block(tcb + c * F, nb, q);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                const f32x4 tdd = r16::load_block(tdb + c * F, nb, q);
                u[c].b[nb] = (tvv[c] + tdd) + ((tkk[c1] * vv[c2] + kk[c1] * tvv[c2]) - (tkk[c2] * vv[c1] + kk[c2] * tvv[c1]));
                if (ok) r16::store_block(tdb + c * F, nb, q, u[c].b[nb]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            OP tve;
            const float tsc = tve.set_tangent(u[c]);
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                f32x4 b0 = Z4, b1 = Z4;
                r16::gemm_bt_sc(b0, b1, tve, tsc, wl, lane);
                tn.b[2 * ch] += stat(c, 2 * ch) * b0; tn.b[2 * ch + 1] += stat(c, 2 * ch + 1) * b1;
                pipe.release();
            }
        }
    }
    // ---- phase B: tangent of MLP([ |vv| , s + ds ])
    A16 tsn;                                        // ts + tds, then ts after the update (phase D's operand): read once, kept in registers
    OP th2;
    float th2sc;
    {
        A16 u;
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) u.b[nb] = Z4;
        {
            OP tnn;
            const float tsc = tnn.set_tangent(tn);
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                r16::gemm_bt_sc(u.b[2 * ch], u.b[2 * ch + 1], tnn, tsc, wl, lane);
                pipe.release();
            }
        }
        {
            OP tss;
#pragma unroll
            for (int nb = 0; nb < NBK; ++nb) tsn.b[nb] = r16::load_block(tsb, nb, q) + r16::load_block(tab, nb, q);
            const float tsc = tss.set_tangent(tsn);
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                r16::gemm_bt_sc(u.b[2 * ch], u.b[2 * ch + 1], tss, tsc, wl, lane);
                pipe.release();
            }
        }
        {
            A16 nn, kk;
#pragma unroll
            for (int nb = 0; nb < NBK; ++nb) { nn.b[nb] = stat(4, nb); kk.b[nb] = stat(5, nb); }
            r16::ln_tangent(u, nn, kk);
        }
        {
            OP th1;
            const float tsc = th1.set_tangent(u);
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                f32x4 b0 = Z4, b1 = Z4;
                r16::gemm_bt_sc(b0, b1, th1, tsc, wl, lane);
                u.b[2 * ch] = b0; u.b[2 * ch + 1] = b1;
                pipe.release();
            }
        }
        {
            A16 nn, kk;
#pragma unroll
            for (int nb = 0; nb < NBK; ++nb) { nn.b[nb] = stat(6, nb); kk.b[nb] = stat(7, nb); }
            r16::ln_tangent(u, nn, kk);
        }
        th2sc = th2.set_tangent(u);
    }
    // ---- output chunks: ts += 2 n n' q + n^2 q' + add'
#pragma unroll
    for (int ch = 0; ch < NB; ++ch) {
        const f32x4* wl = pipe.acquire();
        f32x4 tq0 = Z4, tq1 = Z4;
        r16::gemm_bt_sc(tq0, tq1, th2, th2sc, wl, lane);
        pipe.release();
        wl = pipe.acquire();
        f32x4 ta0 = Z4, ta1 = Z4;
        r16::gemm_bt_sc(ta0, ta1, th2, th2sc, wl, lane);
        pipe.release();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int nb = 2 * ch + k;
            f32x4 so = tsn.b[nb];
            const f32x4 tqq = k ? tq1 : tq0, taa = k ? ta1 : ta0, nrm = stat(3, nb), qq = stat(8, nb);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float n = nrm[r], dn = tn.b[nb][r];
                so[r] = so[r] + (((2.0f * n) * dn) * qq[r] + (n * n) * tqq[r] + taa[r]);
            }
            tsn.b[nb] = so;
            if (ok) {
                r16::store_block(tsb, nb, q, so);
                if (p.zero_acc) r16::store_block(tab, nb, q, Z4);
            }
        }
    }
    A16 tgg;
#pragma unroll
    for (int ch = 0; ch < NB; ++ch) {
        const f32x4* wl = pipe.acquire();
        f32x4 b0 = Z4, b1 = Z4;
        r16::gemm_bt_sc(b0, b1, th2, th2sc, wl, lane);
        tgg.b[2 * ch] = b0; tgg.b[2 * ch + 1] = b1;
        pipe.release();
    }
    // ---- phase C: tv = tv_eff + (U tv_eff) gates + (U v_eff) tgates
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        OP tve;
        A16 u;                                      // the parked tv_eff row: operand and addend, read once
        r16::load_set(u, tdb + c * F, q);
        const float tsc = tve.set_tangent(u);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 b0 = Z4, b1 = Z4;
            r16::gemm_bt_sc(b0, b1, tve, tsc, wl, lane);
            pipe.release();
            if (ok) {
                r16::store_block(tvb + c * F, 2 * ch, q, u.b[2 * ch] + (b0 * stat(9, 2 * ch) + stat(10 + c, 2 * ch) * tgg.b[2 * ch]));
                r16::store_block(tvb + c * F, 2 * ch + 1, q, u.b[2 * ch + 1] + (b1 * stat(9, 2 * ch + 1) + stat(10 + c, 2 * ch + 1) * tgg.b[2 * ch + 1]));
                if (p.zero_acc) {
                    r16::store_block(tdb + c * F, 2 * ch, q, Z4);
                    r16::store_block(tdb + c * F, 2 * ch + 1, q, Z4);
                }
            }
        }
    }
    if (ok && p.zero_acc) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int nb = 0; nb < NBK; ++nb) r16::store_block(tcb + c * F, nb, q, Z4);
    }
    // ---- phase D: tangent of P for the next message block (no bias)
    if (p.has_next) {
        OP sn;
        const float tsc = sn.set_tangent(tsn);      // the rows written above, still in registers
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = Z4, a1 = Z4;
            r16::gemm_bt_sc(a0, a1, sn, tsc, wl, lane);
            pipe.release();
            if (ok) { r16::store_block(p.tP + (size_t)nd * F, 2 * ch, q, a0); r16::store_block(p.tP + (size_t)nd * F, 2 * ch + 1, q, a1); }
        }
    }
    pipe.drain();
}

// ================================================================================================== tangent readout kernel
// tout[vnode][c] = (Vr . tv_c) gate + (Vr . v_c) tgate   (LayerReadout.forward, cpainn.py:425-437)
// The cross-lane sums below are VALU lane swaps (mfma_chain.hpp: xquarters), and that matters here: with ds_bpermute the split
// build of this kernel lost (Vr . v) sums of whole tiles whenever EXEC was narrowed for the store while the permute was still
// outstanding.
template <int NBK, bool SPLIT>
__global__ __launch_bounds__(256, (NBK <= 8 ? 2 : 1)) void painn_jvp_readout_kernel(const JvpReadoutParams p)
{
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = 256 * NB;
    using A16 = r16::Act<NBK>;
    using OP = r16::Opnd<NBK, SPLIT>;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    float* vec = reinterpret_cast<float*>(lds + 4 * CH4);
    for (int i = threadIdx.x; i < RV::COUNT * F / 4; i += T)
        reinterpret_cast<f32x4*>(vec)[i] = reinterpret_cast<const f32x4*>(p.vecs)[i];
    PipeDMA<NB, T, 2> pipe;
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);

    const long long node = ((long long)blockIdx.x * WAVES + wave) * 16 + j;      // virtual node
    const long long nd = node < p.N ? node : p.N - 1;
    const long long vm = nd / p.A, vg = vm / p.G;
    const long long pm_raw = (vg / p.D) * p.G + (vm - vg * p.G);                      // molecule of this virtual molecule
    const bool ok = node < p.N && pm_raw < p.B;
    const size_t pn = (size_t)((pm_raw < p.B ? pm_raw : p.B - 1) * p.A + (nd - vm * p.A));   // primal node

    A16 t, u;
    {
        OP ss, tss;
        float ssc, tsc;
        {
            A16 x, y;
            r16::load_set(x, p.s + pn * F, q);
            r16::load_set(y, p.ts + (size_t)nd * F, q);
            ssc = ss.set_scaled(x); tsc = tss.set_tangent(y);
        }
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = r16::load_block(vec + RV::B0 * F, 2 * ch, q), a1 = r16::load_block(vec + RV::B0 * F, 2 * ch + 1, q);
            f32x4 b0 = Z4, b1 = Z4;
            r16::gemm_bt2_sc(a0, a1, b0, b1, ss, ssc, tss, tsc, wl, lane);
            t.b[2 * ch] = a0; t.b[2 * ch + 1] = a1; u.b[2 * ch] = b0; u.b[2 * ch + 1] = b1;
            pipe.release();
        }
    }
    r16::ln_silu_dual(t, u, vec + RV::G0 * F, vec + RV::BE0 * F, q);
    {
        OP h1, th1;
        h1.set(t);
        const float tsc = th1.set_tangent(u);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = r16::load_block(vec + RV::B1 * F, 2 * ch, q), a1 = r16::load_block(vec + RV::B1 * F, 2 * ch + 1, q);
            f32x4 b0 = Z4, b1 = Z4;
            r16::gemm_bt2_sc(a0, a1, b0, b1, h1, 1.0f, th1, tsc, wl, lane);
            t.b[2 * ch] = a0; t.b[2 * ch + 1] = a1; u.b[2 * ch] = b0; u.b[2 * ch + 1] = b1;
            pipe.release();
        }
    }
    r16::ln_silu_dual(t, u, vec + RV::G1 * F, vec + RV::BE1 * F, q);
    float gate = 0.f, tgate = 0.f;
#pragma unroll
    for (int nb = 0; nb < NBK; ++nb) {
        const f32x4 w = r16::load_block(vec + RV::W2G * F, nb, q);
#pragma unroll
        for (int r = 0; r < 4; ++r) { gate = fmaf(t.b[nb][r], w[r], gate); tgate = fmaf(u.b[nb][r], w[r], tgate); }
    }
    gate = r16::xquarters(gate) + p.b2_gate;
    tgate = r16::xquarters(tgate);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = 0.f, tacc = 0.f;
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) {
            const f32x4 w = r16::load_block(vec + RV::VR * F, nb, q);
            const f32x4 vv = r16::load_block(p.v + (pn * 3 + c) * F, nb, q), tv = r16::load_block(p.tv + ((size_t)nd * 3 + c) * F, nb, q);
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc = fmaf(vv[r], w[r], acc); tacc = fmaf(tv[r], w[r], tacc); }
        }
        acc = r16::xquarters(acc); tacc = r16::xquarters(tacc);
        if (ok && q == 0) p.tout[nd * 3 + c] = tacc * gate + acc * tgate;
    }
    pipe.drain();
}

// div[b] = sum_d tangent[(virtual molecule of (b, d))][d]  (unit seeds: direction d = 3 atom + component is also the flat
// index inside [A][3]); fixed summation order
__global__ void painn_div_reduce_kernel(const float* __restrict__ tout, long long B, int D, int G, float* __restrict__ div)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long long pg = b / G, m = b - pg * G;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc += tout[(size_t)(((pg * D + d) * G + m)) * D + d];
    div[b] = acc;
}

// Hutchinson contraction (include/ti_hip.h ti_painn_drift_div_est): est[b] = (1/k) sum_p sum_i eps[b][p][i] tangent[(b, p)][i] with
// D = k explicit directions.  One wave per molecule: lane l takes the entries i = l, l + 64, ... of probe 0, 1, ... in that order
// (fp64), then a fixed butterfly -- deterministic, and independent of where the molecule sits in the batch.
__global__ void __launch_bounds__(256) painn_hutch_reduce_kernel(const float* __restrict__ tout, const float* __restrict__ eps, long long B,
                                                                int k, int n3, int G, float* __restrict__ est)
{
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;                                             // whole waves leave together
    const long long pg = b / G, m = b - pg * G;
    double acc = 0.0;
    for (int pr = 0; pr < k; ++pr) {
        const float* tg = tout + (size_t)((pg * k + pr) * G + m) * n3;
        const float* ev = eps + (size_t)(b * k + pr) * n3;
        for (int i = lane; i < n3; i += 64) acc += (double)ev[i] * (double)tg[i];
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) est[b] = (float)(acc / k);
}

// ================================================================================================== launchers
static size_t jvp_edge_lds(int NB) { return 4 * (size_t)256 * NB * 16 + 4 * 128 * 4 + EV::COUNT * (size_t)32 * NB * 4; }
static size_t jvp_node_lds(int NB, int count)
{
    return 4 * (size_t)256 * NB * 16 + (size_t)count * 32 * NB * 4;
}

// The five kernels of the family and their builds: every width x SPLIT, the filter and the edge kernel also as masked twins.
enum JvpKernel { JVP_FILTER, JVP_EDGE, JVP_NODE, JVP_UPDATE, JVP_READOUT };
constexpr bool jvp_build_exists(JvpKernel k, bool mask) { return !mask || k == JVP_FILTER || k == JVP_EDGE; }
static size_t jvp_lds_bytes(JvpKernel k, int NB)
{
    return k == JVP_EDGE ? jvp_edge_lds(NB) : jvp_node_lds(NB, k == JVP_FILTER ? EV::COUNT : k == JVP_READOUT ? RV::COUNT : UV::COUNT);
}
template <JvpKernel K, int NBK, bool SPLIT, bool MASK>
constexpr auto jvp_kernel()
{
    if constexpr (K == JVP_FILTER && MASK) return painn_jvp_filter_mask_kernel<NBK, SPLIT>;
    else if constexpr (K == JVP_FILTER) return painn_jvp_filter_kernel<NBK, SPLIT>;
    else if constexpr (K == JVP_EDGE && MASK) return painn_jvp_edge_mask_kernel<NBK, SPLIT>;
    else if constexpr (K == JVP_EDGE) return painn_jvp_edge_kernel<NBK, SPLIT>;
    else if constexpr (K == JVP_NODE) return painn_jvp_node_kernel<NBK, SPLIT>;
    else if constexpr (K == JVP_UPDATE) return painn_jvp_update_kernel<NBK, SPLIT>;
    else return painn_jvp_readout_kernel<NBK, SPLIT>;
}
// The visitor of the family: f(kernel, LDS bytes) for every build of kernel K that the values select (EVERY: all of them, dispatch.hpp),
// until one returns an error.  hipErrorInvalidValue: no such build.
template <JvpKernel K, class F>
static hipError_t with_jvp_builds(int NB, int masked, int split, F&& f)
{
    hipError_t e = hipSuccess;
    bool any = false;
    dispatch_int<1, 2, 4, 8>(NB, [&](auto nc) { dispatch_bool(masked, [&](auto mc) { dispatch_bool(split, [&](auto sc) {
        constexpr int nb = decltype(nc)::value;
        constexpr bool MASK = decltype(mc)::value, SPLIT = decltype(sc)::value;
        if constexpr (jvp_build_exists(K, MASK)) {
            any = true;
            if (e == hipSuccess) e = f(jvp_kernel<K, 2 * nb, SPLIT, MASK>(), jvp_lds_bytes(K, nb));
        }
    }); }); });
    return any ? e : hipErrorInvalidValue;
}
template <JvpKernel K>
static hipError_t configure_jvp(int NB)
{
    return with_jvp_builds<K>(NB, EVERY, EVERY, [](auto kernel, size_t lds) { return set_lds(kernel, lds); });
}
// blocks of 4 waves: one wave per group (filter, edge) or per 16 nodes (node, update, readout)
template <JvpKernel K, class P>
static hipError_t launch_jvp(int NB, bool split, bool masked, long long blocks, const P& p, hipStream_t st)
{
    return with_jvp_builds<K>(NB, masked, split, [&](auto kernel, size_t lds) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, st, p);
        return hipGetLastError();
    });
}

hipError_t configure_painn_jvp_kernels(int NB)
{
    hipError_t e;
    if ((e = configure_jvp<JVP_FILTER>(NB)) != hipSuccess) return e;
    if ((e = configure_jvp<JVP_EDGE>(NB)) != hipSuccess) return e;
    if ((e = configure_jvp<JVP_NODE>(NB)) != hipSuccess) return e;
    if ((e = configure_jvp<JVP_UPDATE>(NB)) != hipSuccess) return e;
    return configure_jvp<JVP_READOUT>(NB);
}

hipError_t launch_jvp_filter(int NB, bool split, const JvpFilterParams& p, hipStream_t st, bool masked)
{
    return launch_jvp<JVP_FILTER>(NB, split, masked, (p.n_groups + 3) / 4, p, st);
}
hipError_t launch_jvp_edge(int NB, bool split, const JvpEdgeParams& p, hipStream_t st, bool masked)
{
    return launch_jvp<JVP_EDGE>(NB, split, masked, (p.n_groups + 3) / 4, p, st);
}
hipError_t launch_jvp_node(int NB, bool split, const JvpNodeParams& p, hipStream_t st) { return launch_jvp<JVP_NODE>(NB, split, false, (p.N + 63) / 64, p, st); }
hipError_t launch_jvp_update(int NB, bool split, const JvpUpdateParams& p, hipStream_t st) { return launch_jvp<JVP_UPDATE>(NB, split, false, (p.N + 63) / 64, p, st); }
hipError_t launch_jvp_readout(int NB, bool split, const JvpReadoutParams& p, hipStream_t st) { return launch_jvp<JVP_READOUT>(NB, split, false, (p.N + 63) / 64, p, st); }

hipError_t launch_div_reduce(const float* tout, long long B, int D, int G, float* div, hipStream_t st)
{
    hipLaunchKernelGGL(painn_div_reduce_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, tout, B, D, G, div);
    return hipGetLastError();
}

hipError_t launch_hutch_reduce(const float* tout, const float* eps, long long B, int k, int A, int G, float* est, hipStream_t st)
{
    hipLaunchKernelGGL(painn_hutch_reduce_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, tout, eps, B, k, 3 * A, G, est);
    return hipGetLastError();
}

}  // namespace ti
