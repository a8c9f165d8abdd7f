// painn_kernels.hip -- cPaiNN drift kernels for gfx950 (MI355X).
//
// Restates (never copies) the arithmetic of the reference modules; citations are relative to /root/reference:
//   embed   : InvariantFeatures/NominalEmbedding/TemperatureEncoder/PositionalEmbedding + CombineInvariantFeatures
//             mdqm9/thermo/ambient/models/embedding.py:68-86,127-160,200-212,249-261 (latent twins)
//   edge    : AddSpatialFeatures graph.py:25-33 + SE3Message.forward cpainn.py:263-310
//   update  : Update.forward cpainn.py:345-376, EquivariantLinear cpainn.py:403
//   readout : LayerReadout.forward cpainn.py:425-437, cPaiNN.forward cpainn.py:112-115
//
// Dense layers run on the matrix cores through mfma_chain.hpp (f32 32x32x2 / 16x16x4, or fp16 16x16x32 with split operands);
// activations never leave registers inside an MLP chain; per-atom sums over incoming edges are formed per 16-row block by a
// selection product and added to HBM accumulators with no-return atomics by the one wave that owns the molecule, in program
// order -- deterministic without an ordered reduction tree.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "dispatch.hpp"
#include "mfma_chain.hpp"
#include "painn_update_kernel.hpp"
#include "ti_internal.hpp"

namespace ti {

// the message kernels live in painn_{edge,pair}[_mask]_nb*.hip (painn_edge_kernel.hpp, painn_pair_kernel.hpp; ti_internal.hpp: *_unit)

// ================================================================================================== update kernel
// v <- v + dv  with  dv = dvacc + cacc x v   (the cross product with v[dst] factors out of the edge sum),
// s <- s + dsacc, then Update.forward (cpainn.py:345-376); finally P for the next layer's message block.
// FOLDED: the message kernel has already added the cross term to dvacc (pair_folds_cross, ti_internal.hpp): dv = dvacc, cacc unused.
// 16 atoms per wave on the r16 primitives (f32 or split-fp16 matrix path), 4 waves per workgroup, 2 workgroups per CU.
// The three spatial components share every visit of the U / V weight chunks.
// (struct UV, update_superchunk, update_chunk4, update_lds_bytes: painn_update_kernel.hpp, shared with painn_update_keep.hip)
template <int NBK, bool HAS_NEXT, int PREC, bool FOLDED = false>
__global__ __launch_bounds__(256, (NBK <= 8 ? 2 : 1)) void painn_update_kernel(const UpdateParams p)
#define TI_UPDATE_SCLS false
#define TI_UPDATE_KEEP 0
#include "painn_update_kernel_body.inc"
#undef TI_UPDATE_SCLS

// layer 0's update after an embed per class (painn_host.hip): s comes in through the class map (painn_update_kernel_body.inc: SCLS)
template <int NBK, bool HAS_NEXT, int PREC = 1, bool FOLDED = false>
__global__ __launch_bounds__(256, (NBK <= 8 ? 2 : 1)) void painn_update_cls_kernel(const UpdateParams p)
#define TI_UPDATE_SCLS true
#include "painn_update_kernel_body.inc"
#undef TI_UPDATE_SCLS
#undef TI_UPDATE_KEEP
// (their twins that keep v_eff in registers: painn_update_keep.hip, a unit of its own so that these code objects stay as they were)

// ================================================================================================== embed / readout kernels
// embed:   s = MLP([atom_emb | enc(T0) | enc(T1) | enc(t)]),  P = s @ phi0.W0[:, :F]^T + phi0.b0
// readout: gate(MLP(s)) * (Vr . v)
// 16 atoms per wave on the r16 primitives and the precision's matrix path (f32 16x16x4, split fp16, fp16).  (Until round 2 these two ran
// 32 rows per wave on the f32 32x32x2 MFMA whatever the precision: a lone wave spent 1.8 us per weight chunk there against 0.3 us here,
// which is what a small batch pays -- 80 + 35 us of a 620 us evaluation of 12 molecules.)
// TV: the time of node nd is p.tv[nd / A] (one time per molecule, the reference's per-node batch.t); else the scalar p.t.
template <int NBK, int NSEG, int PREC, bool TV = false>
__global__ __launch_bounds__(256, (NBK <= 8 ? 2 : 1)) void painn_embed16_kernel(const EmbedParams p)
#define TI_EMBED_REP false
#include "painn_embed_kernel_body.inc"
#undef TI_EMBED_REP

// the embed launch over (class, atom) rows alone (painn_embed_kernel_body.inc: REP)
template <int NBK, int NSEG, int PREC = 1, bool TV = false>
__global__ __launch_bounds__(256, (NBK <= 8 ? 2 : 1)) void painn_embed16_cls_kernel(const EmbedParams p)
#define TI_EMBED_REP true
#include "painn_embed_kernel_body.inc"
#undef TI_EMBED_REP

template <int NBK, int PREC>
__global__ __launch_bounds__(256, (NBK <= 8 ? 2 : 1)) void painn_readout16_kernel(const ReadoutParams p)
{
    constexpr bool H16 = PREC == 2;
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = update_chunk4(NB, H16);
    using A16 = r16::Act<NBK>;
    using OP = typename r16::OpSel<NBK, PREC>::type;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    PipeDMA<NB, T, 2, CH4> pipe;
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);
    const long long node = ((long long)blockIdx.x * WAVES + wave) * 16 + j;
    const bool ok = node < p.N;
    const size_t nd = (size_t)(ok ? node : p.N - 1);

    A16 h1;
    {
        OP sop;
        float ssc;
        {
            A16 ss;
#pragma unroll
            for (int nb = 0; nb < NBK; ++nb) ss.b[nb] = r16::load_state<H16>(p.s, nd * F, nb, q);
            ssc = sop.set_scaled(ss);
        }
        const float sinv = r16::pow2_inverse(ssc);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = r16::load_block(p.mlp.b0, 2 * ch, q) * sinv, a1 = r16::load_block(p.mlp.b0, 2 * ch + 1, q) * sinv;
            r16::gemm_bt(a0, a1, sop, wl, lane);
            h1.b[2 * ch] = a0 * ssc; h1.b[2 * ch + 1] = a1 * ssc;
            pipe.release();
        }
    }
    r16::ln_silu(h1, p.mlp.g0, p.mlp.be0, q);
    A16 h2;
    {
        OP o1;
        o1.set(h1);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = r16::load_block(p.mlp.b1, 2 * ch, q), a1 = r16::load_block(p.mlp.b1, 2 * ch + 1, q);
            r16::gemm_bt(a0, a1, o1, wl, lane);
            h2.b[2 * ch] = a0; h2.b[2 * ch + 1] = a1;
            pipe.release();
        }
    }
    pipe.drain();
    r16::ln_silu(h2, p.mlp.g1, p.mlp.be1, q);
    // split(mlp(s), 1): [invariant_out (unused by cPaiNN.forward), gates]; the 1-row output layers are dot products over the features
    float gate = 0.f;
#pragma unroll
    for (int nb = 0; nb < NBK; ++nb) {
        const f32x4 w = r16::load_block(p.w2_gate, nb, q);
#pragma unroll
        for (int r = 0; r < 4; ++r) gate += h2.b[nb][r] * w[r];
    }
    gate = r16::xquarters(gate) + p.b2_gate;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float vv = 0.f;
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) {
            const f32x4 x = r16::load_state<H16>(p.v, (nd * 3 + c) * F, nb, q), w = r16::load_block(p.Vr, nb, q);
#pragma unroll
            for (int r = 0; r < 4; ++r) vv += x[r] * w[r];
        }
        vv = r16::xquarters(vv);
        if (ok && q == 0) p.out[node * 3 + c] = vv * gate;
    }
}

// ================================================================================================== launchers
static size_t node16_lds_bytes(int NB, bool h16) { return 2 * 2 * (size_t)update_chunk4(NB, h16) * 16; }      // PipeDMA<.., SC = 2>: two superchunks

// The three node kernels and their builds: every width x precision (prec: include/ti_hip.h TI_PREC_*; 0 f32, 1 f16x2, 2 f16 storage
// mode: the state tensors are fp16), and per kernel two more arguments (n, flag):
//   embed16: NSEG = 2, 3, 4 x TV;   update: HAS_NEXT x FOLDED, FOLDED only where the pair kernel folds (pair_folds_cross);   readout: (0, false)
enum NodeKernel { NODE_EMBED, NODE_UPDATE, NODE_READOUT, NODE_EMBED_CLS, NODE_UPDATE_CLS };
// the per-class builds (embed per class and the first update after it): where the layer-0 phi table exists, (n, false) as their twins
constexpr bool node_build_exists(NodeKernel k, int nb, int PREC, int n, bool flag)
{
    if (k == NODE_EMBED_CLS || k == NODE_UPDATE_CLS) return pair_table_build_exists(nb, PREC, false) && !flag && (k == NODE_EMBED_CLS ? n >= 2 : n <= 1);
    return k == NODE_EMBED ? n >= 2 : k == NODE_UPDATE ? n <= 1 && (!flag || pair_folds_cross(PREC)) : n == 0 && !flag;
}
template <NodeKernel K, int NBK, int PREC, int N, bool FLAG>
constexpr auto node_kernel()
{
    if constexpr (K == NODE_EMBED) return painn_embed16_kernel<NBK, N, PREC, FLAG>;
    else if constexpr (K == NODE_UPDATE) return painn_update_kernel<NBK, N != 0, PREC, FLAG>;
    else if constexpr (K == NODE_EMBED_CLS) return painn_embed16_cls_kernel<NBK, N>;
    else if constexpr (K == NODE_UPDATE_CLS) return painn_update_cls_kernel<NBK, N != 0>;
    else return painn_readout16_kernel<NBK, PREC>;
}
// The visitor of the family: f(kernel, LDS bytes) for every build of kernel K that the values select (EVERY: all of them, dispatch.hpp),
// until one returns an error.  hipErrorInvalidValue: no such build.
template <NodeKernel K, class F>
static hipError_t with_node_builds(int NB, int prec, int n, int flag, F&& f)
{
    hipError_t e = hipSuccess;
    bool any = false;
    dispatch_int<1, 2, 4, 8>(NB, [&](auto bc) { dispatch_int<0, 1, 2>(prec, [&](auto pc) { dispatch_int<0, 1, 2, 3, 4>(n, [&](auto nc) { dispatch_bool(flag, [&](auto fc) {
        constexpr int nb = decltype(bc)::value, PREC = decltype(pc)::value, N = decltype(nc)::value;
        constexpr bool FLAG = decltype(fc)::value;
        if constexpr (node_build_exists(K, nb, PREC, N, FLAG)) {
            any = true;
            if (e == hipSuccess) e = f(node_kernel<K, 2 * nb, PREC, N, FLAG>(), K == NODE_UPDATE || K == NODE_UPDATE_CLS ? update_lds_bytes(nb, PREC == 2) : node16_lds_bytes(nb, PREC == 2));
        }
    }); }); }); });
    return any ? e : hipErrorInvalidValue;
}
template <NodeKernel K>
static hipError_t configure_node(int NB)
{
    return with_node_builds<K>(NB, EVERY, EVERY, EVERY, [](auto kernel, size_t lds) { return set_lds(kernel, lds); });
}
template <NodeKernel K, class P>
static hipError_t launch_node(int NB, int prec, int n, bool flag, const P& p, hipStream_t st)
{
    return with_node_builds<K>(NB, prec, n, flag, [&](auto kernel, size_t lds) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((p.N + 63) / 64)), dim3(256), lds, st, p);       // 4 waves x 16 atoms per workgroup
        return hipGetLastError();
    });
}

// f(NB, MASK as constants) for the one-width units of the message kernels that (NB, masked) select
template <class F>
static hipError_t with_message_units(int NB, int masked, F&& f)
{
    hipError_t e = hipSuccess;
    const bool any = dispatch_int<1, 2, 4, 8>(NB, [&](auto bc) { dispatch_bool(masked, [&](auto mc) { if (e == hipSuccess) e = f(bc, mc); }); });
    return any ? e : hipErrorInvalidValue;
}

hipError_t configure_painn_kernels(int NB)
{
    hipError_t e;
    if ((e = configure_node<NODE_EMBED>(NB)) != hipSuccess) return e;
    if ((e = configure_node<NODE_UPDATE>(NB)) != hipSuccess) return e;
    if ((e = configure_node<NODE_READOUT>(NB)) != hipSuccess) return e;
    if ((e = configure_update_keep(NB)) != hipSuccess) return e;
    if (pair_table_build_exists(NB, TI_PREC_F16X2, false)) {
        if ((e = configure_node<NODE_EMBED_CLS>(NB)) != hipSuccess) return e;
        if ((e = configure_node<NODE_UPDATE_CLS>(NB)) != hipSuccess) return e;
    }
    if ((e = configure_phi0_kernels(NB)) != hipSuccess) return e;
    return with_message_units(NB, EVERY, [](auto bc, auto mc) {
        constexpr int nb = decltype(bc)::value;
        constexpr bool MASK = decltype(mc)::value;
        hipError_t e = configure_edge_unit<nb, MASK>();
        if constexpr (pair_build_exists(nb, 4, TI_PREC_F32)) {
            if (e == hipSuccess) e = configure_pair_unit<nb, MASK, false>();
            if constexpr (!MASK) {
                if (e == hipSuccess) e = configure_pair_unit<nb, false, true>();
                if (e == hipSuccess) e = configure_pair_unit<nb, false, false, true>();
                if (e == hipSuccess) e = configure_pair_unit<nb, false, true, true>();
                if (e == hipSuccess) e = configure_pair_tails_unit<nb>();
            }
        }
        return e;
    });
}

hipError_t launch_embed(int NB, int nseg, int prec, const EmbedParams& p, hipStream_t st)
{
    if (p.rep) return p.tv ? hipErrorInvalidValue : launch_node<NODE_EMBED_CLS>(NB, prec, nseg, false, p, st);
    return launch_node<NODE_EMBED>(NB, prec, nseg, p.tv != nullptr, p, st);
}
hipError_t launch_update(int NB, bool has_next, int prec, const UpdateParams& p, hipStream_t st, bool folded, bool keep)
{
    if (keep) return launch_update_keep(NB, has_next, prec, p, st, folded);
    if (p.s_cls) return folded ? hipErrorInvalidValue : launch_node<NODE_UPDATE_CLS>(NB, prec, has_next, false, p, st);
    return launch_node<NODE_UPDATE>(NB, prec, has_next, folded, p, st);
}
hipError_t launch_readout(int NB, int prec, const ReadoutParams& p, hipStream_t st) { return launch_node<NODE_READOUT>(NB, prec, 0, false, p, st); }

hipError_t launch_edge(int NB, bool first, bool last, int prec, const EdgeParams& p, hipStream_t st, bool masked)
{
    return with_message_units(NB, masked, [&](auto bc, auto mc) { return launch_edge_unit<decltype(bc)::value, decltype(mc)::value>(first, last, prec, p, st); });
}
hipError_t launch_pair(int NB, bool first, bool last, int prec, const EdgeParams& p, hipStream_t st, bool masked, bool table, bool seeded)
{
    if (seeded && (masked || !pair_general_build_exists(prec) || p.n_tile <= 0 || p.n_tile >= p.nblk)) return hipErrorInvalidValue;
    return with_message_units(NB, masked, [&](auto bc, auto mc) {
        constexpr int nb = decltype(bc)::value;
        if constexpr (pair_build_exists(nb, 4, TI_PREC_F32)) {
            if (seeded) {          // the general blocks first: they store; the kernel boundary orders the tile launch's adds behind them
                EdgeParams g = p;
                g.row_stride = 0;
                hipError_t e = p.tail_S > 0 ? launch_pair_tails_unit<nb>(first, last, g, st, table) : launch_pair_unit<nb, false, true, true>(first, last, prec, g, st, table);
                return e == hipSuccess ? launch_pair_unit<nb, false, false, true>(first, last, prec, p, st, table) : e;
            }
            hipError_t e = p.n_tile > 0 ? launch_pair_unit<nb, decltype(mc)::value, false>(first, last, prec, p, st, table) : hipSuccess;
            if (e == hipSuccess && p.n_tile < p.nblk) {      // the general blocks: one kernel for shared and per-group row words
                EdgeParams g = p;
                g.row_stride = masked ? p.nblk * 16 : 0;
                e = launch_pair_unit<nb, false, true>(first, last, prec, g, st, table);
            }
            return e;
        } else return hipErrorInvalidValue;
    });
}

}  // namespace ti
