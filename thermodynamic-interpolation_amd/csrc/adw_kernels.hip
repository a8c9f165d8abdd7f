// adw_kernels.hip -- FCNetMultiBeta drift (adw double well) on gfx950, plus the elementwise integrator kernels.
//
// Restates /root/reference/adw/thermo/models/simple.py:22-41.  Both MLPs of the model have the same shape
//   Linear(3 -> H), SiLU, [Linear(H -> H), SiLU] x n_hidden, Linear(H -> 1)
// (beta_embed: inputs [beta0, beta1, t], n_hidden = 1;  net: inputs [x, t, beta_embed], n_hidden = num_layers-1),
// so one kernel serves both: hidden activations stay in registers, H x H layers on the matrix cores.
#include "adw_device.hpp"
#include "dispatch.hpp"
#include "mfma_chain.hpp"
#include "ti_internal.hpp"

namespace ti {

// Per-MLP vector block in LDS (floats): w_in [H][3] | b_in [H] | b_hidden [n_hidden][H] | w_out [H]
//
// 16 rows per wave on the r16 primitives (mfma_chain.hpp), f32 or split-fp16 matrix path.  TAN additionally propagates the
// tangent d/d(a0) through the network (forward mode): out_div = d out / d a0, which for `net` is the divergence of the 1-D
// drift, ODEWrapper.compute_divergence (/root/reference/adw/thermo/models/ode_wrapper.py:55-67) without its 1e-2 factor.
template <int NBK, bool SPLIT, bool TAN>
__global__ __launch_bounds__(256, (NBK <= 8 && !TAN) ? 2 : 1) void adw_mlp_kernel(const AdwParams p)
{
    constexpr int H = 16 * NBK, NB = (H + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = 256 * NB;
    using A16 = r16::Act<NBK>;
    using OP = r16::Opnd<NBK, SPLIT>;
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
    const bool ok = row < p.B;
    const long long r = ok ? row : p.B - 1;
    const float a0 = p.x[r];
    const float a1 = p.in1 ? p.in1[r] : p.t;
    const float a2 = p.idx ? p.emb[p.idx[r]] : (p.emb ? p.emb[r] : p.t);

    // the MLP itself (adw_device.hpp): shared with the fused rollout kernel, one source for both
    float o, d;
    adw_net_eval<NBK, SPLIT, TAN>(pipe, w_in, b_in, b_hid, w_out, p.n_hidden, p.b_out, a0, a1, a2, lane, q, o, d);
    if (ok && q == 0) { p.out[row] = o; if (TAN) p.out_div[row] = d; }
    pipe.drain();
}

// ---- d-dimensional net (FCNetMultiBeta(d, d, H, L), 2 <= d <= 16).  Inputs [x_0 .. x_{d-1}, t, embed], outputs d.
// Vector block (floats): w_in [H][Kpad] (Kpad = d + 2 rounded up to 4, zero columns) | b_in [H] | b_hidden [n_hidden][H] |
// w_out [d][H] | b_out [d] (padded to 4).  The beta embedding stays on adw_mlp_kernel (3 inputs, 1 output).
// TAN: out_div = sum_i d out_i / d x_i, forward mode.  Direction i starts as silu'(z) * W_in[:, i] and needs only output i.  The
// directions run in groups of G (a register budget: G tangent sets + their operands beside the primal's); every group recomputes the
// primal, and each hidden-layer weight chunk from pipe.acquire() feeds the primal and all G tangent products of that chunk.  The
// weight stream is cyclic (PipeDMA), so a group simply streams the hidden layers again.
constexpr int ADW_MAX_DIM = 16, ADW_KMAX4 = (ADW_MAX_DIM + 2 + 3) / 4;
__host__ __device__ constexpr int adw_tan_group(int NBK) { return NBK >= 16 ? 1 : NBK >= 8 ? 2 : NBK >= 4 ? 4 : 8; }

template <int NBK, bool SPLIT, bool TAN, int G>
__global__ __launch_bounds__(256, (NBK <= 8 && !TAN) ? 2 : 1) void adw_mlp_nd_kernel(const AdwParams p)
{
    constexpr int H = 16 * NBK, NB = (H + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = 256 * NB, GT = TAN ? G : 1;
    using A16 = r16::Act<NBK>;
    using OP = r16::Opnd<NBK, SPLIT>;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    const int d = p.dim, kp4 = (d + 5) / 4, Kpad = 4 * kp4;
    float* vec = reinterpret_cast<float*>(lds + 2 * CH4);
    const int nvec4 = ((Kpad + 1 + p.n_hidden + d) * H + 4 * ((d + 3) / 4)) / 4;
    for (int i = threadIdx.x; i < nvec4; i += T) reinterpret_cast<f32x4*>(vec)[i] = reinterpret_cast<const f32x4*>(p.vecs)[i];
    PipeDMA<NB, T, 1> pipe;
    if (p.nch > 0) pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);
    else __syncthreads();
    const float* w_in = vec;
    const float* b_in = vec + Kpad * H;
    const float* b_hid = b_in + H;
    const float* w_out = b_hid + (size_t)p.n_hidden * H;
    const float* b_out = w_out + (size_t)d * H;

    const long long row = ((long long)blockIdx.x * WAVES + wave) * 16 + j;
    const bool ok = row < p.B;
    const long long r = ok ? row : p.B - 1;
    const float a1 = p.in1 ? p.in1[r] : p.t;
    const float a2 = p.idx ? p.emb[p.idx[r]] : (p.emb ? p.emb[r] : p.t);
    float a[4 * ADW_KMAX4];
#pragma unroll
    for (int c = 0; c < 4 * ADW_KMAX4; ++c) a[c] = c < d ? p.x[r * d + c] : c == d ? a1 : c == d + 1 ? a2 : 0.f;

    auto act = [](float z, float& y, float& dy) {
        const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-z));
        y = z * sg;
        dy = fmaf(y, 1.0f - sg, sg);
    };
    float dsum = 0.f;
    for (int g0 = 0; g0 < (TAN ? d : 1); g0 += GT) {
        A16 cur, tan[GT];
        // input layer (K = Kpad): FMAs over whole f32x4 columns, straight into the register layout
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) {
            const f32x4 bb = r16::load_block(b_in, nb, q);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* w = w_in + (size_t)(16 * nb + 4 * q + k) * Kpad;
                float z = bb[k];
#pragma unroll
                for (int c4 = 0; c4 < ADW_KMAX4; ++c4)
                    if (c4 < kp4) {
                        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + 4 * c4);
                        z = fmaf(wv.w, a[4 * c4 + 3], fmaf(wv.z, a[4 * c4 + 2], fmaf(wv.y, a[4 * c4 + 1], fmaf(wv.x, a[4 * c4], z))));
                    }
                float y, dy;
                act(z, y, dy);
                cur.b[nb][k] = y;
                if constexpr (TAN) {
#pragma unroll
                    for (int g = 0; g < GT; ++g) tan[g].b[nb][k] = g0 + g < d ? dy * w[g0 + g] : 0.f;
                }
            }
        }
        // hidden layers
        for (int l = 0; l < p.n_hidden; ++l) {
            OP in, tin[GT];
            in.set(cur);
            if constexpr (TAN) {
#pragma unroll
                for (int g = 0; g < GT; ++g) tin[g].set(tan[g]);
            }
            const float* bias = b_hid + (size_t)l * H;
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                f32x4 z0 = r16::load_block(bias, 2 * ch, q), z1 = r16::load_block(bias, 2 * ch + 1, q);
                r16::gemm_bt(z0, z1, in, wl, lane);
                f32x4 t0[GT], t1[GT];
                if constexpr (TAN) {
#pragma unroll
                    for (int g = 0; g < GT; ++g) {
                        t0[g] = f32x4{0, 0, 0, 0}; t1[g] = f32x4{0, 0, 0, 0};
                        r16::gemm_bt(t0[g], t1[g], tin[g], wl, lane);
                    }
                }
                pipe.release();
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float y0, dy0, y1, dy1;
                    act(z0[k], y0, dy0); cur.b[2 * ch][k] = y0;
                    act(z1[k], y1, dy1); cur.b[2 * ch + 1][k] = y1;
                    if constexpr (TAN) {
#pragma unroll
                        for (int g = 0; g < GT; ++g) { tan[g].b[2 * ch][k] = dy0 * t0[g][k]; tan[g].b[2 * ch + 1][k] = dy1 * t1[g][k]; }
                    }
                }
            }
        }
        // output layer: one dot product per component for the primal (first group only), one per direction for the tangents
        if (g0 == 0) {
            for (int i = 0; i < d; ++i) {
                const float* wo = w_out + (size_t)i * H;
                float o = 0.f;
#pragma unroll
                for (int nb = 0; nb < NBK; ++nb) {
                    const f32x4 w = r16::load_block(wo, nb, q);
#pragma unroll
                    for (int k = 0; k < 4; ++k) o = fmaf(cur.b[nb][k], w[k], o);
                }
                o = r16::xquarters(o) + b_out[i];
                if (ok && q == 0) p.out[row * d + i] = o;
            }
        }
        if constexpr (TAN) {
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                if (g0 + g >= d) break;
                const float* wo = w_out + (size_t)(g0 + g) * H;
#pragma unroll
                for (int nb = 0; nb < NBK; ++nb) {
                    const f32x4 w = r16::load_block(wo, nb, q);
#pragma unroll
                    for (int k = 0; k < 4; ++k) dsum = fmaf(tan[g].b[nb][k], w[k], dsum);
                }
            }
        }
    }
    if constexpr (TAN) {
        dsum = r16::xquarters(dsum);
        if (ok && q == 0) p.out_div[row] = dsum;
    }
    pipe.drain();
}

// floats of the per-MLP vector block: dim 1 (adw_mlp_kernel) w_in [H][3] b_in b_hidden w_out; dim > 1 as adw_mlp_nd_kernel above
static size_t adw_vec_floats(int H, int n_hidden, int dim)
{
    if (dim <= 1) return (size_t)(5 + n_hidden) * H;
    return (size_t)(4 * ((dim + 5) / 4) + 1 + n_hidden + dim) * H + 4 * ((dim + 3) / 4);
}
size_t adw_vec_floats_host(int H, int n_hidden, int dim) { return adw_vec_floats(H, n_hidden, dim); }
static size_t adw_lds_bytes(int NB, int n_hidden, int dim = 1) { return 2 * (size_t)256 * NB * 16 + adw_vec_floats(32 * NB, n_hidden, dim) * 4; }

// The visitor of the family: f(kernel) for every build the values select (EVERY: all of them, dispatch.hpp), until one returns an
// error.  Every width has the 1-D and the d-dimensional net (nd), each x SPLIT x TAN (with the divergence).  hipErrorInvalidValue: no such width.
template <class F>
static hipError_t with_adw_builds(int NB, int nd, int split, int tan, F&& f)
{
    hipError_t e = hipSuccess;
    bool any = false;
    dispatch_int<1, 2, 4, 8>(NB, [&](auto nc) { dispatch_bool(nd, [&](auto dc) { dispatch_bool(split, [&](auto sc) { dispatch_bool(tan, [&](auto tc) {
        constexpr int NBK = 2 * decltype(nc)::value;
        constexpr bool ND = decltype(dc)::value, SPLIT = decltype(sc)::value, TAN = decltype(tc)::value;
        any = true;
        if (e != hipSuccess) return;
        if constexpr (ND) e = f(adw_mlp_nd_kernel<NBK, SPLIT, TAN, adw_tan_group(NBK)>);
        else e = f(adw_mlp_kernel<NBK, SPLIT, TAN>);
    }); }); }); });
    return any ? e : hipErrorInvalidValue;
}

hipError_t configure_adw_kernels(int NB, int max_hidden, int dim)
{
    const size_t bytes = std::max(adw_lds_bytes(NB, max_hidden), adw_lds_bytes(NB, max_hidden, dim));
    return with_adw_builds(NB, EVERY, EVERY, EVERY, [&](auto kernel) { return set_lds(kernel, bytes); });
}

hipError_t launch_adw(int NB, bool split, const AdwParams& p, hipStream_t st)
{
    if (p.dim > ADW_MAX_DIM) return hipErrorInvalidValue;
    const size_t l = adw_lds_bytes(NB, p.n_hidden, p.dim > 1 ? p.dim : 1);
    return with_adw_builds(NB, p.dim > 1, split, p.out_div != nullptr, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((p.B + 63) / 64)), dim3(256), l, st, p);
        return hipGetLastError();
    });
}

// ================================================================================================== integrator
// Unfused multiply/add on purpose: the reference state update is `x + dt * b` in two roundings.
__global__ void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, float a, const float* __restrict__ b, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __fadd_rn(x[i], __fmul_rn(a, b[i]));
}
__global__ void heun_kernel(float* __restrict__ x, float hdt, const float* __restrict__ b1, const float* __restrict__ b2, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = __fadd_rn(x[i], __fmul_rn(hdt, __fadd_rn(b1[i], b2[i])));
}

// Philox4x32-10 / ti_normal: adw_device.hpp (one definition, also drawn inside the fused rollout kernel)

// one thread per trajectory: x[traj][c] += sigma * (xi_c - COM_c)
__global__ void noise_kernel(float* __restrict__ x, float sigma, uint64_t seed, long long traj0, int step, long long B, int comps,
                             int atoms_for_com)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= B) return;
    float com[3] = {0.f, 0.f, 0.f};
    if (atoms_for_com > 0) {
        for (int c = 0; c < comps; ++c) com[c % 3] += ti_normal(seed, traj0 + m, step, c);
        for (int k = 0; k < 3; ++k) com[k] = com[k] / (float)atoms_for_com;
    }
    for (int c = 0; c < comps; ++c) {
        float z = ti_normal(seed, traj0 + m, step, c);
        if (atoms_for_com > 0) z -= com[c % 3];
        x[m * comps + c] = __fadd_rn(x[m * comps + c], __fmul_rn(sigma, z));
    }
}

// Rademacher probes of the Hutchinson estimator (include/ti_hip.h ti_painn_drift_div_est): eps[b][p][i] = sign of
// ti_normal(seed, traj0 + b, p, i) (0 -> +1), i = 3 atom + component -- the component index noise_kernel draws for a molecule.
__global__ void probe_kernel(float* __restrict__ eps, uint64_t seed, long long traj0, long long B, int k, int comps)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * k * comps) return;
    const long long bp = i / comps, b = bp / k;
    const int c = (int)(i - bp * comps), pr = (int)(bp - b * k);
    eps[i] = ti_normal(seed, traj0 + b, pr, c) >= 0.0f ? 1.0f : -1.0f;
}

// ---- mixed-species batches (ti_painn_set_molecules): arrays of [mols][A][comps] floats; molecule i of the array has n_atoms[i / rep]
// real atoms, the atoms behind them are pads
__global__ void park_pads_kernel(float* __restrict__ dst, const float* __restrict__ src, const int32_t* __restrict__ n_atoms, long long mols,
                                 int rep, int A, int comps, int park_coords)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mols * A * comps) return;
    const long long node = i / comps, mol = node / A;
    const int c = (int)(i - node * comps), a = (int)(node - mol * A), n = n_atoms[mol / rep];
    float v = src[i];
    if (a >= n) {
        v = 0.0f;
        if (park_coords) v = __fadd_rn(src[mol * A * comps + c], c == 0 ? 100.0f * (float)(a - n + 1) : 0.0f);      // beside real atom 0
    }
    dst[i] = v;
}
__global__ void zero_pads_kernel(float* __restrict__ y, const int32_t* __restrict__ n_atoms, long long mols, int rep, int A, int comps)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mols * A * comps) return;
    const long long node = i / comps, mol = node / A;
    if ((int)(node - mol * A) >= n_atoms[mol / rep]) y[i] = 0.0f;
}
__global__ void copy_pads_kernel(float* __restrict__ dst, const float* __restrict__ src, const int32_t* __restrict__ n_atoms, long long mols,
                                 int A, int comps)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mols * A * comps) return;
    const long long node = i / comps, mol = node / A;
    if ((int)(node - mol * A) >= n_atoms[mol]) dst[i] = src[i];
}
// noise_kernel over the 3 n_atoms[m] real components of molecule m (rows of [A][3]): the draws (seed, traj, step, 3a + c) a batch of
// its species alone would make, the centre of mass over its real atoms, nothing on pads
__global__ void noise_ragged_kernel(float* __restrict__ x, float sigma, uint64_t seed, long long traj0, int step, long long B, int A, int com_free,
                                    const int32_t* __restrict__ n_atoms)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= B) return;
    const int n = n_atoms[m], comps = 3 * n;
    float com[3] = {0.f, 0.f, 0.f};
    if (com_free) {
        for (int c = 0; c < comps; ++c) com[c % 3] += ti_normal(seed, traj0 + m, step, c);
        for (int k = 0; k < 3; ++k) com[k] = com[k] / (float)n;
    }
    for (int c = 0; c < comps; ++c) {
        float z = ti_normal(seed, traj0 + m, step, c);
        if (com_free) z -= com[c % 3];
        x[m * 3 * A + c] = __fadd_rn(x[m * 3 * A + c], __fmul_rn(sigma, z));
    }
}
// painn_div_reduce_kernel (painn_jvp_kernels.hip) over the real unit seeds: div[b] = sum_{d < 3 n_atoms[b]} tout[(b, d)][d], D = 3A
__global__ void div_reduce_ragged_kernel(const float* __restrict__ tout, long long B, int D, int G, const int32_t* __restrict__ n_atoms,
                                         float* __restrict__ div)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long long pg = b / G, m = b - pg * G;
    const int nd = 3 * n_atoms[b];
    float acc = 0.f;
    for (int d = 0; d < nd; ++d) acc += tout[(size_t)(((pg * D + d) * G + m)) * D + d];
    div[b] = acc;
}

__global__ void scale_kernel(float* __restrict__ y, const float* __restrict__ x, float a, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = x[i] * a;
}

__global__ void nan_check_kernel(const float* __restrict__ x, long long n, int* flag)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !isfinite(x[i])) *flag = 1;
}

// MFMA lane-map self-test: D = A * B with A[i][k] = 1 + i + 100k, B[k][j] = 1000 + j - 7k; also returns the
// accumulator-layout ids so the host can check (reg, lane) -> (row, col) independently.  On the 32x32x2 f32 instruction, which only
// this test still issues.
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__global__ void selftest_kernel(float* out)
{
    const int l = threadIdx.x;
    const float a = 1.0f + (float)(l & 31) + 100.0f * (float)(l >> 5);
    const float b = 1000.0f + (float)(l & 31) - 7.0f * (float)(l >> 5);
    f32x16 acc = {0};
    acc = mfma32(a, b, acc);
    for (int i = 0; i < 16; ++i) out[l * 16 + i] = acc[i];
}

// Operand-split self-test: Opnd<8, true>::set -- the 8-instruction form with its half-register writes (mfma_chain.hpp: split_quad),
// eight quads back to back as in the kernels -- against the plain arithmetic, bit for bit, on values spread over 45 binades (exact
// fp16 values, zeros and fp16-subnormal residuals included).  out[0] counts the halves that differ.
__global__ void split_selftest_kernel(unsigned* out)
{
    const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;
    r16::Act<8> x;
#pragma unroll
    for (int nb = 0; nb < 8; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned h = (gid * 32u + nb * 4u + r) * 2654435761u;
            h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
            const int e = (int)(h % 45u) - 30;                                   // 2^-30 .. 2^14
            const unsigned keep = (h >> 8) % 5u == 0 ? 0x7fe000u : (h >> 8) % 7u == 0 ? 0u : 0x7fffffu;   // some exact fp16 values, some powers of two
            float v = __builtin_bit_cast(float, (unsigned)((e + 127) << 23) | ((h >> 9) & keep));
            if ((h >> 3) % 11u == 0) v = 0.f;
            x.b[nb][r] = (h & 1u) ? -v : v;
        }
    r16::Opnd<8, true> o;
    o.set(x);
    unsigned bad = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const r16::u32x4 hw = __builtin_bit_cast(r16::u32x4, o.hi[m]), lw = __builtin_bit_cast(r16::u32x4, o.lo[m]);     // registers as dwords
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v0 = x.b[2 * m + (k >> 1)][2 * (k & 1)], v1 = x.b[2 * m + (k >> 1)][2 * (k & 1) + 1];
            const _Float16 h0 = (_Float16)v0, h1 = (_Float16)v1;
            const r16::h2 hr{h0, h1}, lr{(_Float16)((v0 - (float)h0) * 2048.0f), (_Float16)((v1 - (float)h1) * 2048.0f)};
            const unsigned dh = hw[k] ^ __builtin_bit_cast(unsigned, hr), dl = lw[k] ^ __builtin_bit_cast(unsigned, lr);
            bad += ((dh & 0xffffu) != 0) + ((dh >> 16) != 0) + ((dl & 0xffffu) != 0) + ((dl >> 16) != 0);
        }
    }
    // the one-accumulator format's split of the same values (Opnd1::quad: unscaled residual, v_fma_mix with the literal -1.0): its own
    // hand-written sequence with the same half-register-write hazard, so its own bit-for-bit check
    r16::Opnd1<8> o1;
    o1.set(x);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const r16::u32x4 hw = __builtin_bit_cast(r16::u32x4, o1.hi[m]), lw = __builtin_bit_cast(r16::u32x4, o1.lo[m]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v0 = x.b[2 * m + (k >> 1)][2 * (k & 1)], v1 = x.b[2 * m + (k >> 1)][2 * (k & 1) + 1];
            const _Float16 h0 = (_Float16)v0, h1 = (_Float16)v1;
            const r16::h2 hr{h0, h1}, lr{(_Float16)(v0 - (float)h0), (_Float16)(v1 - (float)h1)};      // fp16-subnormal residuals included
            const unsigned dh = hw[k] ^ __builtin_bit_cast(unsigned, hr), dl = lw[k] ^ __builtin_bit_cast(unsigned, lr);
            bad += ((dh & 0xffffu) != 0) + ((dh >> 16) != 0) + ((dl & 0xffffu) != 0) + ((dl >> 16) != 0);
        }
    }
    if (bad) atomicAdd(out, bad);
    // The one-accumulator format relies on v_mfma_f32_16x16x32_f16 taking fp16 SUBNORMAL inputs at face value (tools/micro/mfma_denorm.hip).
    // One wave checks it: A = 2^-24 (the smallest subnormal) everywhere, B = 1 -> every output element must be 32 * 2^-24 = 2^-19 exactly.
    if (gid < 64) {
        r16::h8 a, b;
#pragma unroll
        for (int i = 0; i < 8; ++i) { a[i] = __builtin_bit_cast(_Float16, (unsigned short)1); b[i] = (_Float16)1.0f; }
        const f32x4 d = r16::mfma16h(a, b, f32x4{0, 0, 0, 0});
        unsigned wrong = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) wrong += d[r] != 1.9073486328125e-06f;
        if (wrong) atomicAdd(out + 1, wrong);
    }
}

static inline dim3 grid1(long long n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }

hipError_t launch_axpy(float* y, const float* x, float a, const float* b, long long n, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(axpy_kernel, grid1(n, 256), dim3(256), 0, st, y, x, a, b, n);
    return hipGetLastError();
}
hipError_t launch_heun(float* x, float hdt, const float* b1, const float* b2, long long n, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(heun_kernel, grid1(n, 256), dim3(256), 0, st, x, hdt, b1, b2, n);
    return hipGetLastError();
}
hipError_t launch_probes(float* eps, uint64_t seed, long long traj0, long long B, int k, int comps, hipStream_t st)
{
    const long long n = B * k * comps;
    if (n > 0) hipLaunchKernelGGL(probe_kernel, grid1(n, 256), dim3(256), 0, st, eps, seed, traj0, B, k, comps);
    return hipGetLastError();
}
hipError_t launch_noise(float* x, float sigma, uint64_t seed, long long traj0, int step, long long B, int comps, int atoms_for_com,
                        hipStream_t st)
{
    if (B > 0) hipLaunchKernelGGL(noise_kernel, grid1(B, 128), dim3(128), 0, st, x, sigma, seed, traj0, step, B, comps, atoms_for_com);
    return hipGetLastError();
}
hipError_t launch_park_pads(float* dst, const float* src, const int32_t* n_atoms, long long mols, int rep, int A, int comps, int park_coords,
                            hipStream_t st)
{
    const long long n = mols * A * comps;
    if (n > 0) hipLaunchKernelGGL(park_pads_kernel, grid1(n, 256), dim3(256), 0, st, dst, src, n_atoms, mols, rep, A, comps, park_coords);
    return hipGetLastError();
}
hipError_t launch_zero_pads(float* y, const int32_t* n_atoms, long long mols, int rep, int A, int comps, hipStream_t st)
{
    const long long n = mols * A * comps;
    if (n > 0) hipLaunchKernelGGL(zero_pads_kernel, grid1(n, 256), dim3(256), 0, st, y, n_atoms, mols, rep, A, comps);
    return hipGetLastError();
}
hipError_t launch_copy_pads(float* dst, const float* src, const int32_t* n_atoms, long long mols, int A, int comps, hipStream_t st)
{
    const long long n = mols * A * comps;
    if (n > 0) hipLaunchKernelGGL(copy_pads_kernel, grid1(n, 256), dim3(256), 0, st, dst, src, n_atoms, mols, A, comps);
    return hipGetLastError();
}
hipError_t launch_noise_ragged(float* x, float sigma, uint64_t seed, long long traj0, int step, long long B, int A, int com,
                               const int32_t* n_atoms, hipStream_t st)
{
    if (B > 0) hipLaunchKernelGGL(noise_ragged_kernel, grid1(B, 128), dim3(128), 0, st, x, sigma, seed, traj0, step, B, A, com, n_atoms);
    return hipGetLastError();
}
hipError_t launch_div_reduce_ragged(const float* tout, long long B, int D, int G, const int32_t* n_atoms, float* div, hipStream_t st)
{
    if (B > 0) hipLaunchKernelGGL(div_reduce_ragged_kernel, grid1(B, 256), dim3(256), 0, st, tout, B, D, G, n_atoms, div);
    return hipGetLastError();
}
hipError_t launch_scale(float* y, const float* x, float a, long long n, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(scale_kernel, grid1(n, 256), dim3(256), 0, st, y, x, a, n);
    return hipGetLastError();
}
hipError_t launch_selftest(float* out, hipStream_t st)
{
    hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(64), 0, st, out);
    return hipGetLastError();
}
hipError_t launch_split_selftest(unsigned* out, hipStream_t st)
{
    hipLaunchKernelGGL(split_selftest_kernel, dim3(2048), dim3(256), 0, st, out);      // two workgroups' worth of waves on every CU
    return hipGetLastError();
}
hipError_t launch_nan_check(const float* x, long long n, int* flag, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(nan_check_kernel, grid1(n, 256), dim3(256), 0, st, x, n, flag);
    return hipGetLastError();
}

}  // namespace ti
