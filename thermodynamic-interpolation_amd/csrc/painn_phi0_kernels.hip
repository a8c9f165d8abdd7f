// painn_phi0_kernels.hip -- the layer-0 phi table (include/ti_hip.h TI_PHI0_MAX_CLASSES).
//
// Entering the first message layer s is the embedding's output, v is 0 and e = edge_emb[type], so SE3Message's phi branch
// (phi([s[src] | e]), painn_pair_kernel.hpp) is a function of (source atom's embedding inputs, edge type) and sees no coordinate.
// The embedding's inputs are the atom id (the handle's), the molecule's cond rows and the call's t:
//   * painn_phi0_class_kernel gives every molecule of a call a class id -- molecules whose A x ncond cond values are bitwise equal share
//     one -- once per API call, whatever the order of the molecules;
//   * painn_phi0_table_kernel evaluates, after every embed launch, the branch once per (class, atom, edge type) from P of the class's
//     representative (embed per class, painn_host.hip: from the class's rows of P_cls) with the pair kernel's own primitives, operand formats, chain order and product orientations, and writes its
//     three live output slices, bias included, to a table the TABLE builds of the pair kernel read instead of computing them per pair.
// A row's result does not depend on the rows it shares a tile with, so every entry is bit for bit what the pair kernel computes.
#include "painn_edge_kernel.hpp"

namespace ti {

// One thread per molecule.  state[k] is the representative of class k, claimed in slot order with a compare-and-swap: a molecule
// moves past slot k only after it compared unequal with that slot's representative, and two molecules of one new class meet at the
// same empty slot, where the loser of the swap compares equal with the winner.  So every class holds exactly one slot whatever the
// order the threads run in; only the numbering (and who represents a class) depends on it, and nothing downstream does.
// The lanes of a wave walk the slots in lock step (a lane that found its class leaves the loop), so of the lanes that see a slot
// empty only the first one swaps and hands the outcome to the others: one swap per wave and slot instead of 64 on one address.
__global__ __launch_bounds__(256) void painn_phi0_class_kernel(const Phi0ClassParams p)
{
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= p.B) return;
    const uint32_t* const mine = p.cond + (size_t)m * p.words;
    int k = 0;
    for (; k < TI_PHI0_MAX_CLASSES; ++k) {
        int r = __hip_atomic_load(p.state + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (r < 0) {
            const int lead = __builtin_amdgcn_readfirstlane((int)m);      // the first of the lanes that saw the slot empty
            int old = 0;
            if ((int)m == lead) old = atomicCAS(p.state + k, -1, lead);
            old = __builtin_amdgcn_readfirstlane(old);
            if (old < 0 && (int)m == lead) break;               // this molecule represents class k
            r = old < 0 ? lead : old;
        }
        const uint32_t* const other = p.cond + (size_t)r * p.words;
        bool same = true;
        for (int i = 0; i < p.words && same; ++i) same = mine[i] == other[i];
        if (same) break;
    }
    if (k == TI_PHI0_MAX_CLASSES) { p.state[TI_PHI0_MAX_CLASSES] = 1; k = 0; }      // more classes than the cap: the call falls back
    p.cls[m] = (uint8_t)k;
}

// One wave per 16 table rows (row = (class * A + atom) * PHI0_TYPES + type), four waves per workgroup on one weight stream like the
// node kernels: a tile of the pair kernel's phi branch with one operand set instead of two.  Table: [row][ds | scale_edge_dir | de][F]
// fp32 (the de slice absent when layer 0 is also the last).  Stream: phi.W0 (e half), phi.W1, then per 32 output features the ds, de and scale_edge_dir chunks of phi.W2.
template <int NBK, bool LAST>
__global__ __launch_bounds__(256) void painn_phi0_table_kernel(const Phi0TableParams p)
{
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = edge_chunk4(NB, false), SC = 2;
    using A16 = r16::Act<NBK>;
    using OP = r16::Opnd1<NBK>;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    float* vec = reinterpret_cast<float*>(lds + 2 * SC * CH4);                      // [EV::COUNT][F]
    for (int i = threadIdx.x; i < EV::COUNT * F / 4; i += T)
        reinterpret_cast<f32x4*>(vec)[i] = reinterpret_cast<const f32x4*>(p.vecs)[i];
    PipeDMA<NB, T, SC, CH4> pipe;
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);
    const float eps_p0 = 1e-5f * p.wscale[2] * p.wscale[2], eps_p1 = 1e-5f * p.wscale[3] * p.wscale[3], s_p0 = p.wscale[2];

    const int n_rows = p.n_cls * p.A * PHI0_TYPES, row0 = (blockIdx.x * WAVES + wave) * 16;      // rows past the table's end compute its last row and store nothing
    const int row = row0 + j < n_rows ? row0 + j : n_rows - 1;
    const int type = row % PHI0_TYPES, atom = (row / PHI0_TYPES) % p.A, cls = row / (PHI0_TYPES * p.A);
    // the class's P rows: its representative's in the full P, or (no p.state: embed per class) row `cls` of the compact P_cls
    const float* const PI = p.P + ((size_t)(p.state ? p.state[cls] : cls) * p.A + atom) * F;

    OP h2A;
    {
        OP inA;
        A16 tA;
        r16::load_set(tA, p.edge_emb + type * F, q);
        const float scA = inA.set_scaled(tA);
        const float ivA = r16::pow2_inverse(scA) * s_p0;
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            f32x4 a0 = r16::load_block(PI, 2 * c, q) * ivA, a1 = r16::load_block(PI, 2 * c + 1, q) * ivA;
            r16::gemm_on_pipe<false>(a0, a1, inA, pipe, lane);
            tA.b[2 * c] = a0 * scA; tA.b[2 * c + 1] = a1 * scA;
            pipe.release();
        }
        r16::ln_silu(tA, vec + EV::P_G0 * F, vec + EV::P_BE0 * F, q, eps_p0);
        inA.set(tA);
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            f32x4 a0 = r16::load_block(vec + EV::P_B1 * F, 2 * c, q), a1 = r16::load_block(vec + EV::P_B1 * F, 2 * c + 1, q);
            r16::gemm_on_pipe<false>(a0, a1, inA, pipe, lane);
            tA.b[2 * c] = a0; tA.b[2 * c + 1] = a1;
            pipe.release();
        }
        r16::ln_silu(tA, vec + EV::P_G1 * F, vec + EV::P_BE1 * F, q, eps_p1);
        h2A.set(tA);
    }
    // flipped product (ds, scale_edge_dir): lane (n = j, q) register r holds table row row0 + 4q + r of feature 32 nbo + n (and + 16)
    auto flipped = [&](int c, int sl, int nbo) {
        const float* bp = vec + (EV::P_B2 + c) * F + 32 * nbo + j;
        const float p0 = bp[0], p1 = bp[16];
        f32x4 a0 = {p0, p0, p0, p0}, a1 = {p1, p1, p1, p1};
        r16::gemm_on_pipe<true>(a0, a1, h2A, pipe, lane);
        pipe.release();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tr = row0 + 4 * q + r;
            if (tr < n_rows) {
                float* d = p.tab + ((size_t)tr * 3 + sl) * F + 32 * nbo + j;
                d[0] = a0[r]; d[16] = a1[r];
            }
        }
    };
#pragma unroll 1
    for (int nbo = 0; nbo < NB; ++nbo) {
        flipped(2, 0, nbo);
        if constexpr (!LAST) {       // de in the row layout: lane (j, q) holds row j, features 16 (2 nbo) + 4q .. and 16 (2 nbo + 1) + 4q ..
            f32x4 a0 = r16::load_block(vec + (EV::P_B2 + 3) * F, 2 * nbo, q), a1 = r16::load_block(vec + (EV::P_B2 + 3) * F, 2 * nbo + 1, q);
            r16::gemm_on_pipe<false>(a0, a1, h2A, pipe, lane);
            pipe.release();
            if (row0 + j < n_rows) {
                float* d = p.tab + ((size_t)(row0 + j) * 3 + 2) * F;
                r16::store_block(d, 2 * nbo, q, a0); r16::store_block(d, 2 * nbo + 1, q, a1);
            }
        }
        flipped(1, 1, nbo);
    }
    pipe.drain();
}

static size_t phi0_lds_bytes(int NB) { return (size_t)2 * 2 * edge_chunk4(NB, false) * 16 + 21 * (size_t)32 * NB * 4; }

template <class Fn>
static hipError_t with_phi0_builds(int NB, int last, Fn&& f)
{
    hipError_t e = hipSuccess;
    const bool any = dispatch_int<1, 2, 4>(NB, [&](auto bc) { dispatch_bool(last, [&](auto lc) {
        if (e == hipSuccess) e = f(painn_phi0_table_kernel<2 * decltype(bc)::value, decltype(lc)::value>, phi0_lds_bytes(decltype(bc)::value));
    }); });
    return any ? e : hipErrorInvalidValue;
}

hipError_t configure_phi0_kernels(int NB)
{
    if (!pair_table_build_exists(NB, TI_PREC_F16X2, false)) return hipSuccess;      // no table path at this width
    return with_phi0_builds(NB, EVERY, [](auto kernel, size_t lds) { return set_lds(kernel, lds); });
}

hipError_t launch_phi0_classes(const Phi0ClassParams& p, hipStream_t st)
{
    hipLaunchKernelGGL(painn_phi0_class_kernel, dim3((unsigned)((p.B + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_phi0_table(int NB, bool last, const Phi0TableParams& p, hipStream_t st)
{
    const int n_rows = p.n_cls * p.A * PHI0_TYPES;
    return with_phi0_builds(NB, last, [&](auto kernel, size_t lds) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n_rows + 63) / 64)), dim3(256), lds, st, p);
        return hipGetLastError();
    });
}

}  // namespace ti
