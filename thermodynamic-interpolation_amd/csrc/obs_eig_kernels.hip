// obs_eig_kernels.hip -- batched complex-Hermitian fp64 eigensolver in LDS (include/ti_hip.h ti_obs_eigh) and the p x p algebra of
// reversible generator EDMD around it (ti_obs_gedmd_spectrum): whitening, the reduced matrix, the back-transform.
//
// Eigensolver, one 256-thread group per matrix: parallel cyclic two-sided Jacobi.  A and the accumulated V live in LDS as m x m
// complex (re, im) rows, m = n rounded up to even (the pad index never rotates).  A sweep is the m - 1 rounds of the round-robin
// tournament: slot 0 holds index 0, slot k >= 1 holds index 1 + (k - 1 + r) mod (m - 1) in round r, slot i meets slot m - 1 - i.
// A round is three phases with a barrier after each:
//   0  the first m / 2 threads form the rotation of their pair (p, q), p < q, from the matrix as it stands: b = A[p,q], skipped when
//      |b| <= 2^-53 max_k |A_kk of the input|, else tau = (A_qq - A_pp) / (2 |b|), t = sign(tau) / (|tau| + sqrt(1 + tau^2)),
//      c = 1 / sqrt(1 + t^2), s = t c, e = conj(b) / |b|, U = [[c, s], [-s e, c e]] on columns (p, q)
//   1  A <- A U and V <- V U: one item per (row, pair), pairs fastest, so a wave walks distinct columns of one row
//   2  A <- U^H A: one item per (pair, column), columns fastest; the item that holds A[p,q] / A[q,p] stores the exact 0, the one that
//      holds a touched diagonal entry clears its imaginary part
// The iteration stops after the first sweep without a rotation ("something rotated" is a plain LDS store of 1 into the sweep's own
// word).  No atomics: a matrix's result is a function of the matrix alone.  status [i]: the sweep count, -1 for a non-finite entry
// in the triangle that is read (nothing else is written for that matrix), EIG_MAX_SWEEPS + 1 when still rotating after the cap.
#include "ti_internal.hpp"

namespace ti {

namespace {

constexpr int EIG_BLOCK = 256;

struct alignas(16) cplx { double re, im; };
__device__ inline cplx cmul(cplx a, cplx b) { return cplx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

__device__ inline int eig_slot_index(int k, int r, int m) { return k == 0 ? 0 : 1 + (k - 1 + r) % (m - 1); }

// a [n_mat] matrices `mat_stride` doubles apart, row stride ld complex entries; order n, or nvec [i] (0: nothing to do, status 0);
// w [n_mat][ldo], v [n_mat][ldo][ldo] complex or NULL, status [n_mat]
__global__ __launch_bounds__(EIG_BLOCK) void obs_eigh_kernel(const double* __restrict__ a, long long mat_stride, int ld, int n_all,
                                                            const int* __restrict__ nvec, double* __restrict__ w, double* __restrict__ v,
                                                            int ldo, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) double eig_lds[];
    // the tables are kept small on purpose: at n = 50 two groups still share a CU's 160 KiB (2 * 50 * 50 * 16 + 1296 <= 81920).
    // tab: (c, s, Re e, Im e) per pair while rotating, then the diagonal and the ranks; rotated: word sweep % 3 is this sweep's flag
    __shared__ double tab[4 * (EIG_MAX_N / 2)];
    __shared__ int rot_p[EIG_MAX_N / 2], rot_q[EIG_MAX_N / 2], rotated[3], bad;
    double *rot_c = tab, *rot_s = tab + EIG_MAX_N / 2, *rot_er = tab + EIG_MAX_N, *rot_ei = tab + 3 * (EIG_MAX_N / 2);
    const int tid = threadIdx.x;
    const long long mat = blockIdx.x;
    const int n = nvec ? nvec[mat] : n_all;
    if (n < 1 || n > n_all) {                                   // uniform over the group
        if (tid == 0) status[mat] = 0;
        return;
    }
    const int m = n + (n & 1), half = m / 2;
    cplx* A = reinterpret_cast<cplx*>(eig_lds);
    cplx* V = A + m * m;
    const double* __restrict__ src = a + mat * mat_stride;

    if (tid == 0) bad = 0;
    if (tid < 3) rotated[tid] = 0;
    __syncthreads();
    bool ok = true;
    for (int e = tid; e < m * m; e += EIG_BLOCK) {
        const int i = e / m, j = e - i * m;
        cplx x{0.0, 0.0};
        if (i < n && j < n) {
            if (i <= j) {
                x.re = src[2 * ((long long)i * ld + j)];
                x.im = i == j ? 0.0 : src[2 * ((long long)i * ld + j) + 1];
                ok = ok && isfinite(x.re) && isfinite(x.im);
            } else {
                x.re = src[2 * ((long long)j * ld + i)];
                x.im = -src[2 * ((long long)j * ld + i) + 1];
            }
        }
        A[e] = x;
        V[e] = cplx{i == j ? 1.0 : 0.0, 0.0};
    }
    if (!ok) bad = 1;                                          // plain store of one value
    __syncthreads();
    if (bad) {
        if (tid == 0) status[mat] = -1;
        return;
    }
    double scale = 0.0;
    for (int k = 0; k < n; ++k) scale = fmax(scale, fabs(A[k * m + k].re));
    const double thr = 0x1p-53 * scale;

    int sweep = 1;
    for (; sweep <= EIG_MAX_SWEEPS; ++sweep) {
        if (tid == 0) rotated[(sweep + 1) % 3] = 0;           // the next sweep's word: nobody else touches it during this sweep
        for (int r = 0; r < m - 1; ++r) {
            if (tid < half) {
                const int ia = eig_slot_index(tid, r, m), ib = eig_slot_index(m - 1 - tid, r, m);
                const int p = ia < ib ? ia : ib, q = ia < ib ? ib : ia;
                int pp = -1;                                   // -1: no rotation
                if (q < n) {
                    const cplx b = A[p * m + q];
                    const double ab = hypot(b.re, b.im);
                    if (ab > thr) {
                        const double tau = (A[q * m + q].re - A[p * m + p].re) / (2.0 * ab);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        const double c = 1.0 / sqrt(1.0 + t * t);
                        rot_c[tid] = c;
                        rot_s[tid] = t * c;
                        rot_er[tid] = b.re / ab;
                        rot_ei[tid] = -b.im / ab;
                        rot_q[tid] = q;
                        pp = p;
                        rotated[sweep % 3] = 1;
                    }
                }
                rot_p[tid] = pp;
            }
            __syncthreads();
            // columns of A and of V: item = row * half + pair, rows 0 .. m - 1 of A then of V (A and V are contiguous)
            for (int it = tid; it < 2 * m * half; it += EIG_BLOCK) {
                const int row = it / half, k = it - row * half, p = rot_p[k];
                if (p < 0) continue;
                const int q = rot_q[k];
                const double c = rot_c[k], s = rot_s[k];
                const cplx e{rot_er[k], rot_ei[k]}, se{s * e.re, s * e.im}, ce{c * e.re, c * e.im};
                cplx* rowp = A + row * m;
                const cplx xp = rowp[p], xq = rowp[q], u = cmul(se, xq), t2 = cmul(ce, xq);
                rowp[p] = cplx{c * xp.re - u.re, c * xp.im - u.im};
                rowp[q] = cplx{s * xp.re + t2.re, s * xp.im + t2.im};
            }
            __syncthreads();
            // rows of A: item = pair * m + column
            for (int it = tid; it < half * m; it += EIG_BLOCK) {
                const int k = it / m, j = it - k * m, p = rot_p[k];
                if (p < 0) continue;
                const int q = rot_q[k];
                const double c = rot_c[k], s = rot_s[k];
                const cplx ec{rot_er[k], -rot_ei[k]}, se{s * ec.re, s * ec.im}, ce{c * ec.re, c * ec.im};
                const cplx xp = A[p * m + j], xq = A[q * m + j], u = cmul(se, xq), t2 = cmul(ce, xq);
                cplx yp{c * xp.re - u.re, c * xp.im - u.im}, yq{s * xp.re + t2.re, s * xp.im + t2.im};
                if (j == p) { yp.im = 0.0; yq = cplx{0.0, 0.0}; }
                if (j == q) { yq.im = 0.0; yp = cplx{0.0, 0.0}; }
                A[p * m + j] = yp;
                A[q * m + j] = yq;
            }
            __syncthreads();
        }
        if (!rotated[sweep % 3]) break;
    }
    if (sweep > EIG_MAX_SWEEPS) {
        if (tid == 0) status[mat] = EIG_MAX_SWEEPS + 1;
        return;
    }
    // ascending order; equal values by diagonal position: the rank of entry k is the count of entries that come before it
    double* diag = tab;
    int* rank_of = reinterpret_cast<int*>(tab + EIG_MAX_N);
    if (tid < n) diag[tid] = A[tid * m + tid].re;
    __syncthreads();
    if (tid < n) {
        const double dk = diag[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (diag[j] < dk || (diag[j] == dk && j < tid)) ? 1 : 0;
        w[mat * ldo + rank] = dk;
        rank_of[tid] = rank;
    }
    __syncthreads();
    if (v) {
        cplx* __restrict__ vo = reinterpret_cast<cplx*>(v) + mat * ldo * ldo;
        for (int e = tid; e < n * n; e += EIG_BLOCK) {
            const int i = e / n, k = e - i * n;
            vo[(long long)i * ldo + rank_of[k]] = V[i * m + k];
        }
    }
    if (tid == 0) status[mat] = sweep;
}

// s_k = sqrt(max(lambda_k, 0)) of the descending spectrum from the ascending w1 [p]
__device__ inline double gedmd_sval(const double* __restrict__ w1, int p, int k) { return sqrt(fmax(w1[p - 1 - k], 0.0)); }

// The reduced matrix of one Gram matrix per group.  From the eigenpairs (w1 ascending, u1 columns) of G: s descending,
// r = max(#{k : s_k / s_0 >= tol}, nev), L = U[:, :r] / s[:r] in LDS, T = ML L in LDS with ML_ik = (coef K_ik) G_ik (G re-read from
// global memory: its upper triangle, the conjugate below, a real diagonal), then R = L^H T and its Hermitian part, of which the
// upper triangle goes to rmat (row stride p).  rank [i] = r; 0 when the first solve gave no eigenpairs (status1 outside 1 ..
// EIG_MAX_SWEEPS): the second solve and the back-transform then skip the matrix.  A Gram matrix whose kept s holds a 0 (or whose
// largest eigenvalue is not positive) gets a NaN into R[0,0]: the second solve reports it and the back-transform writes NaN.
__global__ __launch_bounds__(EIG_BLOCK) void obs_gedmd_reduce_kernel(const double* __restrict__ gram, const double* __restrict__ w1,
                                                                    const double* __restrict__ u1, const int* __restrict__ status1,
                                                                    const double* __restrict__ kmat, double coef, double tol, int nev, int p,
                                                                    double* __restrict__ rmat, int* __restrict__ rank)
{
    extern __shared__ __attribute__((aligned(16))) double eig_lds[];
    __shared__ double sv[EIG_MAX_N];
    const int tid = threadIdx.x;
    const long long mat = blockIdx.x;
    if (status1[mat] < 1 || status1[mat] > EIG_MAX_SWEEPS) {
        if (tid == 0) rank[mat] = 0;
        return;
    }
    const double* __restrict__ wm = w1 + mat * p;
    const cplx* __restrict__ um = reinterpret_cast<const cplx*>(u1) + mat * p * p;
    const double* __restrict__ g = gram + mat * p * p * 2;
    cplx* __restrict__ R = reinterpret_cast<cplx*>(rmat) + mat * p * p;
    cplx* L = reinterpret_cast<cplx*>(eig_lds);
    cplx* T = L + p * p;
    if (tid < p) sv[tid] = gedmd_sval(wm, p, tid);
    __syncthreads();
    int cnt = 0;
    for (int k = 0; k < p; ++k) cnt += sv[k] / sv[0] >= tol ? 1 : 0;          // a division, then the comparison: NaN counts as below
    const int r = cnt > nev ? cnt : nev;
    if (tid == 0) rank[mat] = r;
    if (!(sv[r - 1] > 0.0)) {                                                 // s is descending: the smallest kept one decides
        if (tid == 0) { R[0].re = __builtin_nan(""); R[0].im = 0.0; }
        return;
    }
    for (int it = tid; it < p * r; it += EIG_BLOCK) {
        const int i = it / r, k = it - i * r;
        const cplx u = um[i * p + (p - 1 - k)];
        L[i * p + k] = cplx{u.re / sv[k], u.im / sv[k]};
    }
    __syncthreads();
    for (int it = tid; it < p * r; it += EIG_BLOCK) {
        const int i = it / r, l = it - i * r;
        cplx acc{0.0, 0.0};
        for (int k = 0; k < p; ++k) {
            const double ck = coef * kmat[i * p + k];
            cplx gk;
            if (i <= k) { gk.re = g[2 * (i * p + k)]; gk.im = i == k ? 0.0 : g[2 * (i * p + k) + 1]; }
            else { gk.re = g[2 * (k * p + i)]; gk.im = -g[2 * (k * p + i) + 1]; }
            const cplx ml{ck * gk.re, ck * gk.im}, x = L[k * p + l];
            acc.re += ml.re * x.re - ml.im * x.im;
            acc.im += ml.re * x.im + ml.im * x.re;
        }
        T[i * p + l] = acc;
    }
    __syncthreads();
    // entry (j, l), j <= l, of the Hermitian part needs R_jl and R_lj: the thread forms both
    for (int it = tid; it < r * r; it += EIG_BLOCK) {
        const int j = it / r, l = it - j * r;
        if (j > l) continue;
        cplx a{0.0, 0.0}, b{0.0, 0.0};
        for (int i = 0; i < p; ++i) {
            const cplx lj = L[i * p + j], ll = L[i * p + l], tj = T[i * p + j], tl = T[i * p + l];
            a.re += lj.re * tl.re + lj.im * tl.im;  a.im += lj.re * tl.im - lj.im * tl.re;       // conj(L_ij) T_il
            b.re += ll.re * tj.re + ll.im * tj.im;  b.im += ll.re * tj.im - ll.im * tj.re;       // conj(L_il) T_ij
        }
        R[j * p + l] = cplx{0.5 * (a.re + b.re), j == l ? 0.0 : 0.5 * (a.im - b.im)};
    }
}

// ev [nev] = the last nev of the second solve's r eigenvalues (ascending), vec [p][nev] = L Wi[:, r - nev:], L formed again from
// (w1, u1) exactly as the reduction formed it; NaN where the second solve refused its matrix (status2 < 0)
__global__ __launch_bounds__(EIG_BLOCK) void obs_gedmd_back_kernel(const double* __restrict__ w1, const double* __restrict__ u1,
                                                                  const double* __restrict__ w2, const double* __restrict__ v2,
                                                                  const int* __restrict__ status2, const int* __restrict__ rank, int nev, int p,
                                                                  double* __restrict__ ev, double* __restrict__ vec)
{
    __shared__ double sv[EIG_MAX_N];
    const int tid = threadIdx.x;
    const long long mat = blockIdx.x;
    const int r = rank[mat], st = status2[mat];
    if (r < nev || r > p || st == 0 || st > EIG_MAX_SWEEPS) return;           // the host refuses the call
    const double* __restrict__ wm = w1 + mat * p;
    const cplx* __restrict__ um = reinterpret_cast<const cplx*>(u1) + mat * p * p;
    const cplx* __restrict__ vm = reinterpret_cast<const cplx*>(v2) + mat * p * p;
    const double nan = __builtin_nan("");
    if (tid < nev) ev[mat * nev + tid] = st < 0 ? nan : w2[mat * p + r - nev + tid];
    if (!vec) return;
    cplx* __restrict__ out = reinterpret_cast<cplx*>(vec) + mat * p * nev;
    if (tid < p) sv[tid] = gedmd_sval(wm, p, tid);
    __syncthreads();
    for (int it = tid; it < p * nev; it += EIG_BLOCK) {
        const int i = it / nev, j = it - i * nev;
        cplx acc{nan, nan};
        if (st > 0) {
            acc = cplx{0.0, 0.0};
            for (int k = 0; k < r; ++k) {
                const cplx u = um[i * p + (p - 1 - k)], x = vm[k * p + (r - nev + j)];
                const cplx l{u.re / sv[k], u.im / sv[k]};
                acc.re += l.re * x.re - l.im * x.im;
                acc.im += l.re * x.im + l.im * x.re;
            }
        }
        out[it] = acc;
    }
}

size_t eig_lds_bytes(int n) { const size_t m = (size_t)n + (n & 1); return 2 * m * m * sizeof(cplx); }

}  // namespace

hipError_t launch_obs_eigh(const double* a, long long mat_stride, int ld, int n, const int* nvec, double* w, double* v, int ldo, int* status,
                           long long n_mat, hipStream_t st)
{
    // more than 64 KiB of dynamic LDS has to be asked for; a group may have all 160 KiB of a CU (128 KiB + tables at n = 64)
    const size_t lds = eig_lds_bytes(n);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(obs_eigh_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)eig_lds_bytes(EIG_MAX_N));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(obs_eigh_kernel, dim3((unsigned)n_mat), dim3(EIG_BLOCK), lds, st, a, mat_stride, ld, n, nvec, w, v, ldo, status);
    return hipGetLastError();
}

hipError_t launch_obs_gedmd_reduce(const double* gram, const double* w1, const double* u1, const int* status1, const double* kmat, double coef,
                                   double tol, int nev, int p, double* rmat, int* rank, long long n_mat, hipStream_t st)
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(obs_gedmd_reduce_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)(2 * (size_t)EIG_MAX_N * EIG_MAX_N * sizeof(cplx)));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(obs_gedmd_reduce_kernel, dim3((unsigned)n_mat), dim3(EIG_BLOCK), 2 * (size_t)p * p * sizeof(cplx), st, gram, w1, u1, status1,
                       kmat, coef, tol, nev, p, rmat, rank);
    return hipGetLastError();
}

hipError_t launch_obs_gedmd_back(const double* w1, const double* u1, const double* w2, const double* v2, const int* status2, const int* rank,
                                 int nev, int p, double* ev, double* vec, long long n_mat, hipStream_t st)
{
    hipLaunchKernelGGL(obs_gedmd_back_kernel, dim3((unsigned)n_mat), dim3(EIG_BLOCK), 0, st, w1, u1, w2, v2, status2, rank, nev, p, ev, vec);
    return hipGetLastError();
}

}  // namespace ti
