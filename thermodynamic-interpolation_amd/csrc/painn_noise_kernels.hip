// painn_noise_kernels.hip -- the base samples of the latent data set on the device (include/ti_hip.h ti_painn_train_noise; the
// reference's mdqm9_latent.py:84-105): x0 = randn_like(x1) per molecule, centred, and with `align` rotated onto x1 by the proper
// rotation that minimises sum_a |x1_a - R x0_a|^2 (scipy's Rotation.align_vectors).  One thread per molecule, everything behind the
// fp32 draw in fp64, a fixed number of Jacobi sweeps in a fixed order, no atomics: a molecule's result is a function of (seed, its
// global index, draw, its x1) alone.  B molecules of at most 32 atoms: the work is a few hundred flops a molecule, bound by launch.
#include "painn_steps.hpp"
#include "adw_device.hpp"
#include "vloss_normal.hpp"

namespace ti {

namespace {

constexpr int PN_BLOCK = 64;
constexpr int PN_SWEEPS = 12;        // cyclic Jacobi on a symmetric 3 x 3 converges quadratically; 6 sweeps reach fp64 round-off

// the Philox normal of (seed, trajectory, draw, component) as vloss_kernels.hip draws z and oracle.normal returns it
__device__ __forceinline__ float pn_normal(uint64_t seed, long long traj, int step, int comp)
{
    uint32_t c[4] = {(uint32_t)traj, (uint32_t)((uint64_t)traj >> 32), (uint32_t)step, (uint32_t)(comp >> 2)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int pair = (comp & 3) >> 1;
    return vl_box_muller(c[2 * pair], c[2 * pair + 1], comp & 1);
}

// one Jacobi rotation of the symmetric m in the (p, q) plane, accumulated into the columns of v
__device__ __forceinline__ void pn_rotate(double (&m)[3][3], double (&v)[3][3], int p, int q)
{
#pragma clang fp contract(off)
    const double apq = m[p][q];
    if (apq == 0.0) return;
    const double theta = (m[q][q] - m[p][p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const int r = 3 - p - q;
    const double app = m[p][p], aqq = m[q][q], arp = m[r][p], arq = m[r][q];
    m[p][p] = app - t * apq; m[q][q] = aqq + t * apq;
    m[p][q] = 0.0; m[q][p] = 0.0;
    m[r][p] = c * arp - s * arq; m[p][r] = m[r][p];
    m[r][q] = s * arp + c * arq; m[q][r] = m[r][q];
    for (int k = 0; k < 3; ++k) {
        const double vp = v[k][p], vq = v[k][q];
        v[k][p] = c * vp - s * vq; v[k][q] = s * vp + c * vq;
    }
}

__device__ __forceinline__ void pn_cross(const double (&a)[3], const double (&b)[3], double (&o)[3])
{
#pragma clang fp contract(off)
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double pn_dot(const double (&a)[3], const double (&b)[3])
{
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// R [3][3] from K = sum_a x1_a x0_a^T
__device__ void pn_kabsch(const double (&K)[3][3], double (&R)[3][3])
{
#pragma clang fp contract(off)
    double m[3][3], v[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += K[k][i] * K[k][j];
            m[i][j] = s; v[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < PN_SWEEPS; ++sweep) { pn_rotate(m, v, 0, 1); pn_rotate(m, v, 0, 2); pn_rotate(m, v, 1, 2); }
    // the columns by descending eigenvalue (ties keep their order)
    int o0 = 0, o1 = 1, o2 = 2;
    if (m[o1][o1] > m[o0][o0]) { const int x = o0; o0 = o1; o1 = x; }
    if (m[o2][o2] > m[o1][o1]) { const int x = o1; o1 = o2; o2 = x; }
    if (m[o1][o1] > m[o0][o0]) { const int x = o0; o0 = o1; o1 = x; }
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3], w[3], v12[3];
    for (int k = 0; k < 3; ++k) { v1[k] = v[k][o0]; v2[k] = v[k][o1]; v3[k] = v[k][o2]; }
    for (int k = 0; k < 3; ++k) u1[k] = K[k][0] * v1[0] + K[k][1] * v1[1] + K[k][2] * v1[2];
    const double n1 = sqrt(pn_dot(u1, u1));
    if (!(n1 > 0.0)) {                          // K = 0 (or not finite): every rotation is a minimiser
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[i][j] = n1 == 0.0 ? (i == j ? 1.0 : 0.0) : n1;
        return;
    }
    for (int k = 0; k < 3; ++k) u1[k] = u1[k] / n1;
    for (int k = 0; k < 3; ++k) u2[k] = K[k][0] * v2[0] + K[k][1] * v2[1] + K[k][2] * v2[2];
    const double d12 = pn_dot(u1, u2);
    for (int k = 0; k < 3; ++k) u2[k] = u2[k] - d12 * u1[k];
    double n2 = sqrt(pn_dot(u2, u2));
    if (!(n2 > 1e-14 * n1)) {                   // rank one (collinear atoms): any unit vector orthogonal to u1
        const int s = fabs(u1[0]) <= fabs(u1[1]) && fabs(u1[0]) <= fabs(u1[2]) ? 0 : fabs(u1[1]) <= fabs(u1[2]) ? 1 : 2;
        double e[3] = {0.0, 0.0, 0.0};
        e[s] = 1.0;
        pn_cross(u1, e, u2);
        n2 = sqrt(pn_dot(u2, u2));
    }
    for (int k = 0; k < 3; ++k) u2[k] = u2[k] / n2;
    pn_cross(u1, u2, u3);
    for (int k = 0; k < 3; ++k) w[k] = K[k][0] * v3[0] + K[k][1] * v3[1] + K[k][2] * v3[2];
    const double su = pn_dot(w, u3) >= 0.0 ? 1.0 : -1.0;           // u_3 of the SVD = su (u1 x u2): det U = su
    pn_cross(v1, v2, v12);
    const double sv = pn_dot(v12, v3) >= 0.0 ? 1.0 : -1.0;         // det V
    const double d = su * sv;                                      // the determinant correction: det(U diag(1, 1, d) V^T) = +1
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = u1[i] * v1[j] + u2[i] * v2[j] + d * (su * u3[i]) * v3[j];
}

__global__ __launch_bounds__(PN_BLOCK) void ptnoise_kernel(const PtNoise p)
{
#pragma clang fp contract(off)
    const long long b = (long long)blockIdx.x * PN_BLOCK + threadIdx.x;
    if (b >= p.B) return;
    const int A = p.A, m = 3 * A;
    double* xc = p.xc + b * m;
    double s[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < A; ++a)
        for (int c = 0; c < 3; ++c) {
            const double x = (double)pn_normal(p.seed, p.traj0 + b, p.draw, 3 * a + c);
            xc[3 * a + c] = x;
            s[c] = s[c] + x;
        }
    for (int c = 0; c < 3; ++c) s[c] = s[c] / (double)A;
    for (int a = 0; a < A; ++a)
        for (int c = 0; c < 3; ++c) xc[3 * a + c] = xc[3 * a + c] - s[c];
    float* out = p.out_x0 + b * m;
    if (!p.aligned) {
        for (int k = 0; k < m; ++k) out[k] = (float)xc[k];
        return;
    }
    const float* x1 = p.x1 + b * m;
    double K[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, R[3][3];
    for (int a = 0; a < A; ++a)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) K[i][j] = K[i][j] + (double)x1[3 * a + i] * xc[3 * a + j];
    pn_kabsch(K, R);
    for (int a = 0; a < A; ++a)
        for (int i = 0; i < 3; ++i)
            out[3 * a + i] = (float)(R[i][0] * xc[3 * a] + R[i][1] * xc[3 * a + 1] + R[i][2] * xc[3 * a + 2]);
    if (p.out_rot)
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) p.out_rot[b * 9 + 3 * i + j] = R[i][j];
}

}  // namespace

hipError_t launch_ptnoise(const PtNoise& p, hipStream_t st)
{
    hipLaunchKernelGGL(ptnoise_kernel, dim3((unsigned)((p.B + PN_BLOCK - 1) / PN_BLOCK)), dim3(PN_BLOCK), 0, st, p);
    return hipGetLastError();
}

}  // namespace ti
