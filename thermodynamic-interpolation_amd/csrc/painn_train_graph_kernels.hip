// painn_train_graph_kernels.hip -- the molecule trainer on per-molecule graphs (include/ti_hip.h ti_painn_train_set_graphs): masked /
// ragged twins of the kernels of a training step that read the graph or run over a molecule's entries -- the velocity loss's
// interpolate, centre and reduce kernels as the trainer uses them (vloss_kernels.hip), and painn_train_kernels.hip's embedding inputs,
// edge embedding, message combine forward and reverse, output gradient and edge-type table -- with the kernel that expands the table
// rows of a call into what they read.  Each twin is its parent's body, statement for statement, with a predicate on what is skipped:
// where nothing is dead and nothing is a pad it evaluates the parent's expressions in the parent's order.
//
// One thread per (row, feature) like the parents; no atomics.  A dead edge row or a pad node row is kept finite in the forward pass
// and given exactly +0 where it would enter a sum of the reverse pass; the dense products and column sums are the untouched kernels.
#include "painn_train_graph.hpp"
#include "adw_device.hpp"
#include "vloss_normal.hpp"

namespace ti {

namespace {

constexpr int PG_BLOCK = 256;
constexpr float PG_PI = 3.14159265358979323846f;
constexpr double PG_PI_D = 3.14159265358979323846;
constexpr uint8_t PG_DEAD = 0x80;

unsigned pg_blocks(long long n) { return (unsigned)((n + PG_BLOCK - 1) / PG_BLOCK); }

__device__ __forceinline__ long long pg_index() { return (long long)blockIdx.x * PG_BLOCK + threadIdx.x; }

__global__ __launch_bounds__(PG_BLOCK) void ptg_expand_kernel(uint8_t* __restrict__ flag, int32_t* __restrict__ nat, const PtTable t,
                                                              const int32_t* __restrict__ etype, const PtGraph g, long long B)
{
    const long long i = pg_index();
    if (i >= B * g.E) return;
    const long long b = i / g.E;
    const int k = (int)(i - b * g.E);
    long long row = t.idx ? t.idx[b] : b;
    if (row < 0 || row >= t.n) row = 0;
    const int n = t.n_atoms[row], s = g.src[k], d = g.dst[k];
    const bool live = s < n && d < n && ((t.mask[row * g.A + d] >> (unsigned)s) & 1u) != 0u;
    const int type = t.ptype ? (int)t.ptype[(row * g.A + s) * g.A + d] : etype[k];
    flag[i] = (uint8_t)((type & 3) | (live ? 0 : PG_DEAD));
    if (k == 0) nat[b] = n;
}

// ---------------------------------------------------------------------------------------------- the velocity loss's kernels
__device__ __forceinline__ double pg_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

constexpr double PG_SIG_SCALE = (double)2.2f;
__device__ __forceinline__ void pg_gamma(int kind, double a, double t, double& g, double& gd)
{
    if (kind == TI_GAMMA_BROWNIAN) {
        g = sqrt(a * t * (1.0 - t));
        gd = a * (1.0 - 2.0 * t) / (2.0 * g);
    } else if (kind == TI_GAMMA_SIN2) {
        const double s = sin(PG_PI_D * t), c = cos(PG_PI_D * t);
        g = s * s;
        gd = 2.0 * PG_PI_D * s * c;
    } else {
        const double sp = pg_sigmoid(a * (t - 0.5) + 1.0), sm = pg_sigmoid(a * (t - 0.5) - 1.0);
        g = PG_SIG_SCALE * (sp - sm - pg_sigmoid(1.0 - 0.5 * a) + pg_sigmoid(-1.0 - 0.5 * a));
        gd = PG_SIG_SCALE * a * ((1.0 - sp) * sp - (1.0 - sm) * sm);
    }
}

__device__ __forceinline__ float pg_normal(uint64_t seed, long long traj, int step, int comp)
{
    uint32_t c[4] = {(uint32_t)traj, (uint32_t)((uint64_t)traj >> 32), (uint32_t)step, (uint32_t)(comp >> 2)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int pair = (comp & 3) >> 1;
    return vl_box_muller(c[2 * pair], c[2 * pair + 1], comp & 1);
}

__global__ __launch_bounds__(PG_BLOCK) void ptg_interp_kernel(VlossParams p, const PtLive lv)
{
    const long long n = p.B * p.m, i = (long long)blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long b = i / p.m;
    const int comp = (int)(i - b * p.m);
    const bool two = p.kind != TI_VLOSS_ONE_SIDED;
    if (comp >= (p.m / p.A) * lv.nat[b]) {                              // a pad entry: nothing is read, nothing is drawn
        if (two) p.z[i] = 0.0f;
        if (p.center != TI_CENTER_NONE) { p.raw[i] = 0.0; if (two) p.raw[n + i] = 0.0; }
        return;
    }
    const double t = (double)p.t[b], x0 = (double)p.x0[i], x1 = (double)p.x1[i];
    double xp, xm = 0.0;
    if (p.kind == TI_VLOSS_ONE_SIDED) xp = t * x1 + (1.0 - t) * x0;
    else {
        const float z = p.z_in ? p.z_in[i] : pg_normal(p.seed, p.traj0 + b, p.draw, comp);
        p.z[i] = z;
        double g, gd;
        pg_gamma(p.gamma, p.a, t, g, gd);
        const double it = (1.0 - t) * x0 + t * x1, gz = g * (double)z;
        xp = it + gz; xm = it - gz;
    }
    if (p.center == TI_CENTER_NONE) { p.xt[i] = (float)xp; if (two) p.xt[p.half + i] = (float)xm; }
    else { p.raw[i] = xp; if (two) p.raw[n + i] = xm; }
}

// blockIdx.y: the half (plus, minus)
__global__ __launch_bounds__(PG_BLOCK) void ptg_center_kernel(VlossParams p, const PtLive lv)
{
    const long long n = p.B * p.m, i = (long long)blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int half = blockIdx.y, nc = p.m / p.A;
    const long long b = i / p.m;
    const int nb = lv.nat[b];
    if ((int)(i - b * p.m) >= nc * nb) return;                 // a pad entry: launch_ptg_pad writes it
    const int c = (int)(i - b * p.m) % nc;
    const double* raw = p.raw + (size_t)half * n;
    double mean;
    if (p.center == TI_CENTER_BATCH) mean = p.colsum[half * nc + c] / lv.N;
    else {
        double s = 0.0;
        for (int a = 0; a < nb; ++a) s += raw[b * p.m + a * nc + c];
        mean = s / (double)nb;
    }
    p.xt[(size_t)half * p.half + i] = (float)(raw[i] - mean);
}

// one thread per (half, molecule, atom)
__global__ __launch_bounds__(PG_BLOCK) void ptg_pad_kernel(float* __restrict__ xt, long long half, int halves, int A, const PtLive lv)
{
    const long long i = pg_index();
    if (i >= (long long)halves * lv.B * A) return;
    const long long r = i / A, hf = r / lv.B, b = r - hf * lv.B;
    const int a = (int)(i - r * A), nb = lv.nat[b];
    if (a < nb) return;
    float* x = xt + hf * half + b * 3 * A;
    x[3 * a] = x[0] + 100.0f * (float)(a - nb + 1); x[3 * a + 1] = x[1]; x[3 * a + 2] = x[2];
}

__global__ __launch_bounds__(PG_BLOCK) void ptg_reduce_kernel(VlossParams p, const PtLive lv)
{
#pragma clang fp contract(off)
    const long long b = (long long)blockIdx.x * PG_BLOCK + threadIdx.x;
    if (b >= p.B) return;
    const long long o = b * p.m;
    const int m = (p.m / p.A) * lv.nat[b];
    const bool two = p.kind != TI_VLOSS_ONE_SIDED;
    double g = 0.0, gd = 0.0;
    if (two) pg_gamma(p.gamma, p.a, (double)p.t[b], g, gd);
    double acc = 0.0;
    for (int k = 0; k < m; ++k) {
        const double d = (double)p.x1[o + k] - (double)p.x0[o + k], bp = (double)p.b[o + k];
        acc += 0.5 * bp * bp;
        if (two) {
            const double gz = gd * (double)p.z[o + k], bm = (double)p.b[p.half + o + k];
            acc -= (d + gz) * bp;
            acc += 0.5 * bm * bm;
            acc -= (d - gz) * bm;
        } else acc -= d * bp;
    }
    p.loss[b] = acc;
}

__device__ __forceinline__ double pg_gamma_dot(int kind, double a, double t)
{
    if (kind == TI_GAMMA_BROWNIAN) return a * (1.0 - 2.0 * t) / (2.0 * sqrt(a * t * (1.0 - t)));
    if (kind == TI_GAMMA_SIN2) return 2.0 * PG_PI_D * sin(PG_PI_D * t) * cos(PG_PI_D * t);
    const double sp = pg_sigmoid(a * (t - 0.5) + 1.0), sm = pg_sigmoid(a * (t - 0.5) - 1.0);
    return (double)2.2f * a * ((1.0 - sp) * sp - (1.0 - sm) * sm);
}

__global__ __launch_bounds__(PG_BLOCK) void ptg_gout_kernel(float* __restrict__ gz, const VlossParams p, const PtLive lv)
{
#pragma clang fp contract(off)
    const long long n = p.B * p.m, i = pg_index();
    if (i >= n) return;
    const long long b = i / p.m;
    if ((int)(i - b * p.m) >= (p.m / p.A) * lv.nat[b]) {       // a pad entry
        gz[i] = 0.0f;
        if (p.kind != TI_VLOSS_ONE_SIDED) gz[n + i] = 0.0f;
        return;
    }
    const double d = (double)p.x1[i] - (double)p.x0[i], inv = lv.N;
    if (p.kind == TI_VLOSS_ONE_SIDED) { gz[i] = (float)(((double)p.b[i] - d) / inv); return; }
    const double gzv = pg_gamma_dot(p.gamma, p.a, (double)p.t[b]) * (double)p.z[i];
    gz[i] = (float)(((double)p.b[i] - (d + gzv)) / inv);
    gz[n + i] = (float)(((double)p.b[p.half + i] - (d - gzv)) / inv);
}

// ---------------------------------------------------------------------------------------------- the trainer's graph kernels
// feature f of PositionalEncoder: cos, sin interleaved per k = f / 2 + 1
__device__ __forceinline__ float pg_posenc(float x_over_len, int f)
{
    const float arg = (x_over_len * (float)(f / 2 + 1)) * PG_PI;
    return (f & 1) ? sinf(arg) : cosf(arg);
}

__global__ __launch_bounds__(PG_BLOCK) void ptg_embed_in_kernel(float* __restrict__ s_in, const PtEmbedIn e, const PtGraph g, const PtLive lv)
{
    const int K = e.nE * g.F;
    const long long i = pg_index();
    if (i >= g.R * g.A * K) return;
    const long long n = i / K, r = n / g.A, b = r % e.B;
    const int j = (int)(i - n * K), a = (int)(n - r * g.A), seg = j / g.F, f = j - seg * g.F;
    float v;
    if (seg == 0) v = e.atom_emb[(size_t)e.atom_ids[a] * g.F + f];
    else if (seg < e.nE - 1) {
        float u = (a < lv.nat[b] ? e.cond[(b * g.A + a) * e.ncond + (seg - 1)] : 0.0f) - e.temp_mean;
        u = u / e.temp_range;
        v = pg_posenc(u / e.temp_length, f);
    } else v = pg_posenc(e.t[b] / e.time_length, f);
    s_in[i] = v;
}

__global__ __launch_bounds__(PG_BLOCK) void ptg_edge_emb_kernel(float* __restrict__ e0, const float* __restrict__ table, const PtGraph g, const PtLive lv)
{
    const long long i = pg_index();
    if (i >= g.R * g.E * g.F) return;
    const long long row = i / g.F, r = row / g.E;
    const int type = lv.flag[(r % lv.B) * g.E + (row - r * g.E)] & 3;
    e0[i] = table[(size_t)type * g.F + (i - row * g.F)];
}

__global__ __launch_bounds__(PG_BLOCK) void ptg_msg_fwd_kernel(float* __restrict__ s_out, float* __restrict__ v_out, const float* __restrict__ s,
                                                               const float* __restrict__ v, const float* __restrict__ P, const float* __restrict__ Wd,
                                                               const float* __restrict__ dir, const PtGraph g, const PtLive lv)
{
    const int F = g.F;
    const long long i = pg_index();
    if (i >= g.R * g.A * F) return;
    const long long n = i / F, r = n / g.A;
    const int f = (int)(i - n * F), a = (int)(n - r * g.A);
    const uint8_t* fl = lv.flag + (r % lv.B) * g.E;
    const float vn0 = v[(n * 3) * F + f], vn1 = v[(n * 3 + 1) * F + f], vn2 = v[(n * 3 + 2) * F + f];
    float ds = 0.f, dv0 = 0.f, dv1 = 0.f, dv2 = 0.f;
    for (int k = 0; k < g.E; ++k) {
        if (g.dst[k] != a || (fl[k] & PG_DEAD)) continue;
        const long long row = r * g.E + k, ns = r * g.A + g.src[k], o = row * 5 * F + f;
        const float gates = P[o] * Wd[o], scale = P[o + F] * Wd[o + F], cross = P[o + 4 * F] * Wd[o + 4 * F];
        const float d0 = dir[3 * row], d1 = dir[3 * row + 1], d2 = dir[3 * row + 2];
        const float c0 = d1 * vn2 - d2 * vn1, c1 = d2 * vn0 - d0 * vn2, c2 = d0 * vn1 - d1 * vn0;
        dv0 += scale * d0 + gates * v[(ns * 3) * F + f] + cross * c0;
        dv1 += scale * d1 + gates * v[(ns * 3 + 1) * F + f] + cross * c1;
        dv2 += scale * d2 + gates * v[(ns * 3 + 2) * F + f] + cross * c2;
        ds += P[o + 2 * F] * Wd[o + 2 * F];
    }
    s_out[i] = s[i] + ds;
    v_out[(n * 3) * F + f] = vn0 + dv0; v_out[(n * 3 + 1) * F + f] = vn1 + dv1; v_out[(n * 3 + 2) * F + f] = vn2 + dv2;
}

__global__ __launch_bounds__(PG_BLOCK) void ptg_msg_bwd_edge_kernel(float* __restrict__ gP, float* __restrict__ gWd, const float* __restrict__ gs,
                                                                    const float* __restrict__ gv, const float* __restrict__ ge, const float* __restrict__ v,
                                                                    const float* __restrict__ P, const float* __restrict__ Wd, const float* __restrict__ dir,
                                                                    const PtGraph g, const PtLive lv)
{
    const int F = g.F;
    const long long i = pg_index();
    if (i >= g.R * g.E * F) return;
    const long long row = i / F, r = row / g.E;
    const int f = (int)(i - row * F), k = (int)(row - r * g.E);
    const long long ns = r * g.A + g.src[k], nd = r * g.A + g.dst[k], o = row * 5 * F + f;
    if (lv.flag[(r % lv.B) * g.E + k] & PG_DEAD) {             // a dead edge: +0 into every product and column sum behind it
#pragma unroll
        for (int j = 0; j < 5; ++j) { gP[o + j * F] = 0.0f; gWd[o + j * F] = 0.0f; }
        return;
    }
    const float g0 = gv[(nd * 3) * F + f], g1 = gv[(nd * 3 + 1) * F + f], g2 = gv[(nd * 3 + 2) * F + f];
    const float s0 = v[(ns * 3) * F + f], s1 = v[(ns * 3 + 1) * F + f], s2 = v[(ns * 3 + 2) * F + f];
    const float t0 = v[(nd * 3) * F + f], t1 = v[(nd * 3 + 1) * F + f], t2 = v[(nd * 3 + 2) * F + f];
    const float d0 = dir[3 * row], d1 = dir[3 * row + 1], d2 = dir[3 * row + 2];
    const float c0 = d1 * t2 - d2 * t1, c1 = d2 * t0 - d0 * t2, c2 = d0 * t1 - d1 * t0;
    float gh[5];
    gh[0] = g0 * s0 + g1 * s1 + g2 * s2;                // gates
    gh[1] = g0 * d0 + g1 * d1 + g2 * d2;                // scale
    gh[2] = gs[nd * F + f];                             // ds
    gh[3] = ge ? ge[row * F + f] : 0.0f;                // de
    gh[4] = g0 * c0 + g1 * c1 + g2 * c2;                // cross gates
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        gP[o + j * F] = gh[j] * Wd[o + j * F];
        gWd[o + j * F] = gh[j] * P[o + j * F];
    }
}

__global__ __launch_bounds__(PG_BLOCK) void ptg_msg_bwd_node_kernel(float* __restrict__ gs_out, float* __restrict__ gv_out, const float* __restrict__ gs,
                                                                    const float* __restrict__ gv, const float* __restrict__ gin_phi,
                                                                    const float* __restrict__ P, const float* __restrict__ Wd, const float* __restrict__ dir,
                                                                    const PtGraph g, const PtLive lv)
{
    const int F = g.F;
    const long long i = pg_index();
    if (i >= g.R * g.A * F) return;
    const long long n = i / F, r = n / g.A;
    const int f = (int)(i - n * F), a = (int)(n - r * g.A);
    const uint8_t* fl = lv.flag + (r % lv.B) * g.E;
    const float g0 = gv[(n * 3) * F + f], g1 = gv[(n * 3 + 1) * F + f], g2 = gv[(n * 3 + 2) * F + f];
    float as = gs[i], a0 = g0, a1 = g1, a2 = g2;
    for (int k = 0; k < g.E; ++k) {
        if (fl[k] & PG_DEAD) continue;
        const long long row = r * g.E + k, o = row * 5 * F + f;
        if (g.src[k] == a) {                                               // an outgoing edge: s[src] of phi's input, gates v[src]
            const long long nd = r * g.A + g.dst[k];
            const float gates = P[o] * Wd[o];
            as += gin_phi[row * 2 * F + f];
            a0 += gates * gv[(nd * 3) * F + f]; a1 += gates * gv[(nd * 3 + 1) * F + f]; a2 += gates * gv[(nd * 3 + 2) * F + f];
        }
        if (g.dst[k] == a) {
            const float cross = P[o + 4 * F] * Wd[o + 4 * F];              // an incoming edge: cross (dir x v[dst]) -> cross (g x dir)
            const float d0 = dir[3 * row], d1 = dir[3 * row + 1], d2 = dir[3 * row + 2];
            a0 += cross * (g1 * d2 - g2 * d1); a1 += cross * (g2 * d0 - g0 * d2); a2 += cross * (g0 * d1 - g1 * d0);
        }
    }
    gs_out[i] = as;
    gv_out[(n * 3) * F + f] = a0; gv_out[(n * 3 + 1) * F + f] = a1; gv_out[(n * 3 + 2) * F + f] = a2;
}

// pt_table_kernel with each molecule's own type per edge; a dead edge belongs to no table row
constexpr int PG_TAB_ACC = 16;
__global__ __launch_bounds__(64 * PG_TAB_ACC) void ptg_table_kernel(double* __restrict__ out, const float* __restrict__ g, long long ld, const PtGraph gr,
                                                                    const PtLive lv)
{
#pragma clang fp contract(off)
    __shared__ double sm[PG_TAB_ACC][64];
    const int F = gr.F, per = gr.E;
    const int c = threadIdx.x & 63, p = threadIdx.x >> 6, f = blockIdx.x * 64 + c, id = blockIdx.y;
    double s = 0.0;
    if (f < F)
        for (long long r = p; r < gr.R; r += PG_TAB_ACC) {
            const uint8_t* fl = lv.flag + (r % lv.B) * per;
            for (int a = 0; a < per; ++a)
                if ((int)fl[a] == id) s = s + (double)g[(r * per + a) * ld + f];
        }
    sm[p][c] = s;
    __syncthreads();
    if (p == 0 && f < F) {
        double t = 0.0;
        for (int q = 0; q < PG_TAB_ACC; ++q) t = t + sm[q][c];
        out[(size_t)id * F + f] = t;
    }
}

}  // namespace

#define PG_LAUNCH(kernel, count, ...) do { hipLaunchKernelGGL(kernel, dim3(pg_blocks(count)), dim3(PG_BLOCK), 0, st, __VA_ARGS__); return hipGetLastError(); } while (0)

hipError_t launch_ptg_expand(uint8_t* flag, int32_t* nat, const PtTable& t, const int32_t* etype, const PtGraph& g, long long B, hipStream_t st)
{
    PG_LAUNCH(ptg_expand_kernel, B * g.E, flag, nat, t, etype, g, B);
}
hipError_t launch_ptg_interp(const VlossParams& p, const PtLive& lv, hipStream_t st) { PG_LAUNCH(ptg_interp_kernel, p.B * p.m, p, lv); }
hipError_t launch_ptg_center(const VlossParams& p, const PtLive& lv, hipStream_t st)
{
    hipLaunchKernelGGL(ptg_center_kernel, dim3(pg_blocks(p.B * p.m), p.kind == TI_VLOSS_ONE_SIDED ? 1 : 2), dim3(PG_BLOCK), 0, st, p, lv);
    return hipGetLastError();
}
hipError_t launch_ptg_pad(float* xt, long long half, int halves, int A, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_pad_kernel, (long long)halves * lv.B * A, xt, half, halves, A, lv);
}
hipError_t launch_ptg_reduce(const VlossParams& p, const PtLive& lv, hipStream_t st) { PG_LAUNCH(ptg_reduce_kernel, p.B, p, lv); }
hipError_t launch_ptg_gout(float* gz, const VlossParams& p, const PtLive& lv, hipStream_t st) { PG_LAUNCH(ptg_gout_kernel, p.B * p.m, gz, p, lv); }
hipError_t launch_ptg_embed_in(float* s_in, const PtEmbedIn& e, const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_embed_in_kernel, g.R * g.A * e.nE * g.F, s_in, e, g, lv);
}
hipError_t launch_ptg_edge_emb(float* e0, const float* table, const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_edge_emb_kernel, g.R * g.E * g.F, e0, table, g, lv);
}
hipError_t launch_ptg_msg_fwd(float* s_out, float* v_out, const float* s, const float* v, const float* P, const float* Wd, const float* dir,
                              const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_msg_fwd_kernel, g.R * g.A * g.F, s_out, v_out, s, v, P, Wd, dir, g, lv);
}
hipError_t launch_ptg_msg_bwd_edge(float* gP, float* gWd, const float* gs, const float* gv, const float* ge, const float* v, const float* P,
                                   const float* Wd, const float* dir, const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_msg_bwd_edge_kernel, g.R * g.E * g.F, gP, gWd, gs, gv, ge, v, P, Wd, dir, g, lv);
}
hipError_t launch_ptg_msg_bwd_node(float* gs_out, float* gv_out, const float* gs, const float* gv, const float* gin_phi, const float* P,
                                   const float* Wd, const float* dir, const PtGraph& g, const PtLive& lv, hipStream_t st)
{
    PG_LAUNCH(ptg_msg_bwd_node_kernel, g.R * g.A * g.F, gs_out, gv_out, gs, gv, gin_phi, P, Wd, dir, g, lv);
}
hipError_t launch_ptg_table(double* out, const float* g, long long ld, const PtGraph& gr, const PtLive& lv, hipStream_t st)
{
    hipLaunchKernelGGL(ptg_table_kernel, dim3((unsigned)((gr.F + 63) / 64), 4u), dim3(64 * PG_TAB_ACC), 0, st, out, g, ld, gr, lv);
    return hipGetLastError();
}

}  // namespace ti
