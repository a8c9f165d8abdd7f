// obs_eig_wide_kernels.hip -- batched complex-Hermitian fp64 eigensolver for orders 64 < n <= 1024 from global memory (include/ti_hip.h
// ti_obs_eigh_wide) and the p x p algebra of reversible generator EDMD around it (ti_obs_gedmd_spectrum_wide).
//
// Blocked two-sided Jacobi.  A and the accumulated V are n x n complex (re, im) rows in buffers of the handle.  Blocks are 32 indices
// wide (nb = ceil(n / 32), the last may be narrow, mb = nb rounded up to even); an outer sweep is the mb - 1 rounds of ti_obs_eigh's
// tournament over block slots, a pair that holds the pad block is skipped.  A round is three launches, and the kernel boundaries are
// the only synchronisation between workgroups:
//   pair    one 1024-thread group per (matrix, block pair I < J): gathers S = A[idx, idx] (idx = the <= 64 indices of I then J) into
//           LDS, applies ONE sweep of ti_obs_eigh's cyclic Jacobi to it with the matrix's own threshold, U accumulated from the
//           identity; writes U and the swept block, the pair's "rotated" word, and a plain 1 into the matrix's word when it rotated
//   column  one group per (matrix, pair, 64-row tile of A or of V): rows <- rows U on the columns idx
//   row     one group per (matrix, pair, 64-column tile of A): rows idx <- U^H rows; the entries inside idx x idx take the swept block
// A pair that did not rotate leaves the matrix alone (its U is the identity and its block is unchanged), so its update groups exit.
// The updates are (64 x 64)(64 x 64) complex products from LDS as four real products on v_mfma_f64_16x16x4_f64 (the instruction of the
// Gram kernels), a wave per 16 output rows, k ascending four at a time.
// No atomics; a matrix's result is a function of the matrix alone.
#include "ti_internal.hpp"

namespace ti {

namespace {

constexpr int EIGW_THREADS = 256;
// the pair kernel holds a CU alone (128 KiB of LDS) and its rounds are short phases between barriers: sixteen waves hide their latency
constexpr int EIGW_PAIR_THREADS = 1024;

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct alignas(16) cplx { double re, im; };
__device__ inline cplx cmul(cplx a, cplx b) { return cplx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

__device__ __forceinline__ int eigw_slot_index(int k, int r, int m) { return k == 0 ? 0 : 1 + (k - 1 + r) % (m - 1); }

// the order of matrix `mat`; below 65 the blocked solver does not take it
__device__ __forceinline__ int eigw_order(const EigWide& e, long long mat) { return e.nvec ? e.nvec[mat] : e.n; }

// The block pair of slot `slot` in round r for a matrix of order n: none (cj = 0) when the slot is beyond the matrix's own tournament, the
// round is beyond its own sweep, or the pair holds the pad block.  i0, j0: first index of I and of J; cj: width of J (I is full).
struct EigwPair { int i0, j0, cj; };                              // cj = 0: no pair
__device__ __forceinline__ EigwPair eigw_pair(int n, int slot, int r)
{
    const int nb = (n + EIGW_BLK - 1) / EIGW_BLK, mb = nb + (nb & 1);
    if (slot >= mb / 2 || r >= mb - 1) return EigwPair{0, 0, 0};
    const int ia = eigw_slot_index(slot, r, mb), ib = eigw_slot_index(mb - 1 - slot, r, mb);
    const int I = ia < ib ? ia : ib, J = ia < ib ? ib : ia;
    if (J >= nb) return EigwPair{0, 0, 0};
    const int j0 = J * EIGW_BLK;
    return EigwPair{I * EIGW_BLK, j0, n - j0 < EIGW_BLK ? n - j0 : EIGW_BLK};
}

// position a of idx (0 .. 32 + cj - 1) -> matrix index
__device__ __forceinline__ int eigw_idx(int a, int i0, int j0) { return a < EIGW_BLK ? i0 + a : j0 + (a - EIGW_BLK); }

__global__ __launch_bounds__(EIGW_THREADS) void eigw_init_kernel(EigWide e, const double* __restrict__ a, long long mat_stride, int lda)
{
    __shared__ double red[EIGW_THREADS];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const long long mat = blockIdx.x;
    const int n = eigw_order(e, mat), ld = e.n;
    if (tid == 0) e.rot[mat] = 0;
    if (n <= EIG_MAX_N || n > e.n) {                               // uniform over the group
        if (tid == 0) e.status[mat] = -2;
        return;
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    const double* __restrict__ src = a + mat * mat_stride;
    cplx* __restrict__ A = reinterpret_cast<cplx*>(e.A) + mat * ld * ld;
    cplx* __restrict__ V = reinterpret_cast<cplx*>(e.V) + mat * ld * ld;
    bool ok = true;
    double scale = 0.0;
    for (int el = tid; el < n * n; el += EIGW_THREADS) {
        const int i = el / n, j = el - i * n;
        cplx x;
        if (i <= j) {
            x.re = src[2 * ((long long)i * lda + j)];
            x.im = i == j ? 0.0 : src[2 * ((long long)i * lda + j) + 1];
            ok = ok && isfinite(x.re) && isfinite(x.im);
            if (i == j) scale = fmax(scale, fabs(x.re));
        } else {
            x.re = src[2 * ((long long)j * lda + i)];
            x.im = -src[2 * ((long long)j * lda + i) + 1];
        }
        A[(long long)i * ld + j] = x;
        V[(long long)i * ld + j] = cplx{i == j ? 1.0 : 0.0, 0.0};
    }
    if (!ok) bad = 1;                                              // plain store of one value
    red[tid] = scale;
    __syncthreads();
    for (int s = EIGW_THREADS / 2; s > 0; s >>= 1) {               // a maximum: exact in any order
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        e.thr[mat] = 0x1p-53 * red[0];
        e.status[mat] = bad ? -1 : 0;
    }
}

// One sweep of obs_eigh_kernel's Jacobi on the gathered block: the same rounds, rotation formulas, exact zeros and real diagonal.
__global__ __launch_bounds__(EIGW_PAIR_THREADS) void eigw_pair_kernel(EigWide e, int r)
{
    extern __shared__ __attribute__((aligned(16))) double eigw_lds[];
    __shared__ double tab[4 * (EIGW_PAIR / 2)];
    __shared__ int rot_p[EIGW_PAIR / 2], rot_q[EIGW_PAIR / 2], rotated;
    double *rot_c = tab, *rot_s = tab + EIGW_PAIR / 2, *rot_er = tab + EIGW_PAIR, *rot_ei = tab + 3 * (EIGW_PAIR / 2);
    const int tid = threadIdx.x, slot = blockIdx.x, nslot = gridDim.x;
    const long long mat = blockIdx.y;
    if (e.status[mat] != 0) return;                                // finished, refused or skipped: uniform over the group
    const int nmat = eigw_order(e, mat), ld = e.n;
    const EigwPair pr = eigw_pair(nmat, slot, r);
    const int i0 = pr.i0, j0 = pr.j0, cj = pr.cj;
    if (cj == 0) {
        if (tid == 0) e.prot[mat * nslot + slot] = 0;
        return;
    }
    const int n = EIGW_BLK + cj, m = n + (n & 1), half = m / 2;
    cplx* A = reinterpret_cast<cplx*>(eigw_lds);
    cplx* V = A + m * m;
    const cplx* __restrict__ G = reinterpret_cast<const cplx*>(e.A) + mat * ld * ld;
    if (tid == 0) rotated = 0;
    for (int el = tid; el < m * m; el += EIGW_PAIR_THREADS) {
        const int i = el / m, j = el - i * m;
        double xr = 0.0, xi = 0.0;
        if (i < n && j < n) {
            const cplx g = G[(long long)eigw_idx(i, i0, j0) * ld + eigw_idx(j, i0, j0)];
            xr = g.re; xi = g.im;
        }
        A[el] = cplx{xr, xi};
        V[el] = cplx{i == j ? 1.0 : 0.0, 0.0};
    }
    __syncthreads();
    const double thr = e.thr[mat];

    for (int rr = 0; rr < m - 1; ++rr) {
        if (tid < half) {
            const int ia = eigw_slot_index(tid, rr, m), ib = eigw_slot_index(m - 1 - tid, rr, m);
            const int p = ia < ib ? ia : ib, q = ia < ib ? ib : ia;
            int pp = -1;                                           // -1: no rotation
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
                    rotated = 1;
                }
            }
            rot_p[tid] = pp;
        }
        __syncthreads();
        for (int it = tid; it < 2 * m * half; it += EIGW_PAIR_THREADS) {
            const int row = it / half, k = it - row * half, p = rot_p[k];
            if (p < 0) continue;
            const int q = rot_q[k];
            const double c = rot_c[k], s = rot_s[k];
            const cplx ee{rot_er[k], rot_ei[k]}, se{s * ee.re, s * ee.im}, ce{c * ee.re, c * ee.im};
            cplx* rowp = A + row * m;
            const cplx xp = rowp[p], xq = rowp[q], u = cmul(se, xq), t2 = cmul(ce, xq);
            rowp[p] = cplx{c * xp.re - u.re, c * xp.im - u.im};
            rowp[q] = cplx{s * xp.re + t2.re, s * xp.im + t2.im};
        }
        __syncthreads();
        for (int it = tid; it < half * m; it += EIGW_PAIR_THREADS) {
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
    const int did = rotated;
    if (tid == 0) {
        e.prot[mat * nslot + slot] = did;
        if (did) e.rot[mat] = 1;                                   // plain store of one value
    }
    if (!did) return;
    cplx* __restrict__ Uo = reinterpret_cast<cplx*>(e.U) + (mat * nslot + slot) * (EIGW_PAIR * EIGW_PAIR);
    cplx* __restrict__ So = reinterpret_cast<cplx*>(e.S) + (mat * nslot + slot) * (EIGW_PAIR * EIGW_PAIR);
    for (int el = tid; el < n * n; el += EIGW_PAIR_THREADS) {
        const int i = el / n, j = el - i * n;
        Uo[i * EIGW_PAIR + j] = V[i * m + j];
        So[i * EIGW_PAIR + j] = A[i * m + j];
    }
}

// ROW = false: X = M[rows of tile][idx] (M = A for tiles < ntile, V after), M[rows][idx] <- X U
// ROW = true:  X = A[idx][columns of tile], A[idx][columns] <- U^H X, and the swept block inside idx x idx
// out (a, b) = sum_k op(P[k][a]) Q[k][b] as real products on v_mfma_f64_16x16x4_f64, k ascending four at a time:
//   column: P[k][a] = X[row a][k] (the tile is stored transposed), Q = U;   row: P = U conjugated, Q[k][b] = X[k][column b]
template <bool ROW>
__global__ __launch_bounds__(EIGW_THREADS) void eigw_update_kernel(EigWide e, int r, int ntile)
{
    extern __shared__ __attribute__((aligned(16))) double eigw_lds[];
    const int tid = threadIdx.x, tile = blockIdx.x, slot = blockIdx.y, nslot = gridDim.y;
    const long long mat = blockIdx.z;
    if (e.status[mat] != 0) return;
    if (!e.prot[mat * nslot + slot]) return;                       // the pair kernel wrote it for every slot of a live matrix
    const int nmat = eigw_order(e, mat), ld = e.n;
    const EigwPair pr = eigw_pair(nmat, slot, r);
    const int i0 = pr.i0, j0 = pr.j0, cj = pr.cj;
    if (cj == 0) return;
    const int n = EIGW_BLK + cj;
    const int t0 = (tile < ntile ? tile : tile - ntile) * EIGW_PAIR;                 // first row (column) of the tile
    if (t0 >= nmat) return;
    const int tw = nmat - t0 < EIGW_PAIR ? nmat - t0 : EIGW_PAIR;                    // rows (columns) of the tile
    cplx* __restrict__ M = reinterpret_cast<cplx*>(!ROW && tile >= ntile ? e.V : e.A) + mat * ld * ld;
    const cplx* __restrict__ Ug = reinterpret_cast<const cplx*>(e.U) + (mat * nslot + slot) * (EIGW_PAIR * EIGW_PAIR);
    cplx* Ul = reinterpret_cast<cplx*>(eigw_lds);
    cplx* Xl = Ul + EIGW_PAIR * EIGW_PAIR;
    for (int el = tid; el < EIGW_PAIR * EIGW_PAIR; el += EIGW_THREADS) {
        const int k = el / EIGW_PAIR, c = el - k * EIGW_PAIR;
        double ur = 0.0, ui = 0.0, xr = 0.0, xi = 0.0;
        if (k < n && c < n) { const cplx u = Ug[el]; ur = u.re; ui = u.im; }
        Ul[el] = cplx{ur, ui};
        if (ROW) {                                                 // Xl[k][column]
            if (k < n && c < tw) { const cplx x = M[(long long)eigw_idx(k, i0, j0) * ld + t0 + c]; xr = x.re; xi = x.im; }
            Xl[el] = cplx{xr, xi};
        } else {                                                   // k = row of the tile, c = position in idx; stored as Xl[c][row]
            if (k < tw && c < n) { const cplx x = M[(long long)(t0 + k) * ld + eigw_idx(c, i0, j0)]; xr = x.re; xi = x.im; }
            Xl[c * EIGW_PAIR + k] = cplx{xr, xi};
        }
    }
    __syncthreads();
    // wave v owns the output rows a = 16 v .. 16 v + 15 and all four 16-column tiles; one K step is four indices k0 + (lane >> 4):
    // re += p.re q.re, re += (-p.im) q.im, im += p.re q.im, im += p.im q.re, in this order (p conjugated first for the row update)
    const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    const cplx* P = ROW ? Ul : Xl;
    const cplx* Q = ROW ? Xl : Ul;
    const int na = ROW ? n : tw, nbk = ROW ? tw : n;               // valid output rows and columns
    f64x4 re[4], im[4];
    for (int t = 0; t < 4; ++t) { re[t] = f64x4{0.0, 0.0, 0.0, 0.0}; im[t] = f64x4{0.0, 0.0, 0.0, 0.0}; }
    if (16 * wave < na) {                                          // uniform over the wave
        for (int k0 = 0; k0 < n; k0 += 4) {                        // rows of P and Q beyond n hold zeros
            const cplx pa = P[(k0 + lq) * EIGW_PAIR + 16 * wave + lr];
            const double pr_ = pa.re, pi_ = ROW ? -pa.im : pa.im;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (16 * t >= nbk) continue;                       // uniform over the group
                const cplx qb = Q[(k0 + lq) * EIGW_PAIR + 16 * t + lr];
                re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr_, qb.re, re[t], 0, 0, 0);
                re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pi_, qb.im, re[t], 0, 0, 0);
                im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr_, qb.im, im[t], 0, 0, 0);
                im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pi_, qb.re, im[t], 0, 0, 0);
            }
        }
    }
    // C / D layout of the instruction: register i of a lane holds row (lane >> 4) + 4 i, column lane & 15 of the tile
    const cplx* __restrict__ Sg = reinterpret_cast<const cplx*>(e.S) + (mat * nslot + slot) * (EIGW_PAIR * EIGW_PAIR);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = 16 * wave + lq + 4 * i, b = 16 * t + lr;
            if (a >= na || b >= nbk) continue;
            double yr = re[t][i], yi = im[t][i];
            if (ROW) {
                const int col = t0 + b;
                if (col >= i0 && col < i0 + EIGW_BLK) { const cplx sv = Sg[a * EIGW_PAIR + (col - i0)]; yr = sv.re; yi = sv.im; }
                else if (col >= j0 && col < j0 + cj) { const cplx sv = Sg[a * EIGW_PAIR + EIGW_BLK + (col - j0)]; yr = sv.re; yi = sv.im; }
                M[(long long)eigw_idx(a, i0, j0) * ld + col] = cplx{yr, yi};
            } else {
                M[(long long)(t0 + a) * ld + eigw_idx(b, i0, j0)] = cplx{yr, yi};
            }
        }
}

__global__ void eigw_sweep_end_kernel(EigWide e, int sweep)
{
    const long long mat = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (mat >= e.n_mat) return;
    if (e.status[mat] == 0) {
        if (!e.rot[mat]) e.status[mat] = sweep;
        else if (sweep >= EIG_MAX_SWEEPS) e.status[mat] = EIG_MAX_SWEEPS + 1;
    }
    e.rot[mat] = 0;
}

// ascending order; equal values by diagonal position: the rank of entry k is the count of entries that come before it
__global__ __launch_bounds__(EIGW_THREADS) void eigw_finish_kernel(EigWide e, double* __restrict__ w, double* __restrict__ v, int ldo)
{
    __shared__ double diag[EIGW_MAX_N];
    __shared__ int rank_of[EIGW_MAX_N];
    const int tid = threadIdx.x;
    const long long mat = blockIdx.x;
    const int st = e.status[mat];
    if (st == -2) {
        if (tid == 0) e.status[mat] = 0;
        return;
    }
    if (st < 1 || st > EIG_MAX_SWEEPS) return;
    const int n = eigw_order(e, mat), ld = e.n;
    const cplx* __restrict__ A = reinterpret_cast<const cplx*>(e.A) + mat * ld * ld;
    const cplx* __restrict__ V = reinterpret_cast<const cplx*>(e.V) + mat * ld * ld;
    for (int k = tid; k < n; k += EIGW_THREADS) diag[k] = A[(long long)k * ld + k].re;
    __syncthreads();
    for (int k = tid; k < n; k += EIGW_THREADS) {
        const double dk = diag[k];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (diag[j] < dk || (diag[j] == dk && j < k)) ? 1 : 0;
        w[mat * ldo + rank] = dk;
        rank_of[k] = rank;
    }
    __syncthreads();
    if (!v) return;
    cplx* __restrict__ vo = reinterpret_cast<cplx*>(v) + mat * ldo * ldo;
    for (int el = tid; el < n * n; el += EIGW_THREADS) {
        const int i = el / n, k = el - i * n;
        vo[(long long)i * ldo + rank_of[k]] = V[(long long)i * ld + k];
    }
}

// ---- the wide gEDMD algebra: what obs_gedmd_reduce_kernel / obs_gedmd_back_kernel define, from global memory

__global__ __launch_bounds__(EIGW_THREADS) void eigw_gedmd_rank_kernel(const double* __restrict__ w1, const double* __restrict__ u1,
                                                                      const int* __restrict__ status1, double tol, int nev, int p,
                                                                      double* __restrict__ s, double* __restrict__ L, double* __restrict__ rmat,
                                                                      int* __restrict__ rank, int* __restrict__ nv_narrow, int* __restrict__ nv_wide,
                                                                      int* __restrict__ live)
{
    __shared__ double sv[EIGW_MAX_N];
    __shared__ int cnts[EIGW_THREADS];
    const int tid = threadIdx.x;
    const long long mat = blockIdx.x;
    if (status1[mat] < 1 || status1[mat] > EIG_MAX_SWEEPS) {
        if (tid == 0) { rank[mat] = 0; nv_narrow[mat] = 0; nv_wide[mat] = 0; live[mat] = 0; }
        return;
    }
    const double* __restrict__ wm = w1 + mat * p;
    const cplx* __restrict__ um = reinterpret_cast<const cplx*>(u1) + mat * p * p;
    for (int k = tid; k < p; k += EIGW_THREADS) {
        sv[k] = sqrt(fmax(wm[p - 1 - k], 0.0));
        s[mat * p + k] = sv[k];
    }
    __syncthreads();
    int cnt = 0;
    for (int k = tid; k < p; k += EIGW_THREADS) cnt += sv[k] / sv[0] >= tol ? 1 : 0;         // a division, then the comparison
    cnts[tid] = cnt;
    __syncthreads();
    for (int h = EIGW_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) cnts[tid] += cnts[tid + h];
        __syncthreads();
    }
    cnt = cnts[0];
    const int r = cnt > nev ? cnt : nev;
    const bool good = sv[r - 1] > 0.0;                             // s is descending: the smallest kept one decides
    if (tid == 0) {
        rank[mat] = r;
        nv_narrow[mat] = r <= EIG_MAX_N ? r : 0;
        nv_wide[mat] = r <= EIG_MAX_N ? 0 : r;
        live[mat] = good ? 1 : 0;
        if (!good) {
            cplx* R = reinterpret_cast<cplx*>(rmat) + mat * p * p;
            R[0].re = __builtin_nan(""); R[0].im = 0.0;
        }
    }
    if (!good) return;
    cplx* __restrict__ Lm = reinterpret_cast<cplx*>(L) + mat * p * p;
    for (int it = tid; it < p * r; it += EIGW_THREADS) {
        const int i = it / r, k = it - i * r;
        const cplx u = um[(long long)i * p + (p - 1 - k)];
        Lm[(long long)i * p + k] = cplx{u.re / sv[k], u.im / sv[k]};
    }
}

// T[i][l] = sum_k (coef K_ik) G_ik L[k][l], l < r: one thread per entry, k ascending
__global__ __launch_bounds__(EIGW_THREADS) void eigw_gedmd_t_kernel(const double* __restrict__ gram, const double* __restrict__ kmat, double coef,
                                                                   const double* __restrict__ L, const int* __restrict__ rank,
                                                                   const int* __restrict__ live, int p, double* __restrict__ T)
{
    const long long mat = blockIdx.y;
    if (!live[mat]) return;
    const int r = rank[mat];
    const long long it = (long long)blockIdx.x * EIGW_THREADS + threadIdx.x;
    if (it >= (long long)p * r) return;
    const int i = (int)(it / r), l = (int)(it - (long long)i * r);
    const double* __restrict__ g = gram + mat * p * p * 2;
    const cplx* __restrict__ Lm = reinterpret_cast<const cplx*>(L) + mat * p * p;
    cplx acc{0.0, 0.0};
    for (int k = 0; k < p; ++k) {
        const double ck = coef * kmat[(long long)i * p + k];
        cplx gk;
        if (i <= k) { gk.re = g[2 * ((long long)i * p + k)]; gk.im = i == k ? 0.0 : g[2 * ((long long)i * p + k) + 1]; }
        else { gk.re = g[2 * ((long long)k * p + i)]; gk.im = -g[2 * ((long long)k * p + i) + 1]; }
        const cplx ml{ck * gk.re, ck * gk.im}, x = Lm[(long long)k * p + l];
        acc.re += ml.re * x.re - ml.im * x.im;
        acc.im += ml.re * x.im + ml.im * x.re;
    }
    reinterpret_cast<cplx*>(T)[mat * p * p + (long long)i * p + l] = acc;
}

// entry (j, l), j <= l, of the Hermitian part of R = L^H T: the thread forms R_jl and R_lj, i ascending
__global__ __launch_bounds__(EIGW_THREADS) void eigw_gedmd_r_kernel(const double* __restrict__ L, const double* __restrict__ T,
                                                                   const int* __restrict__ rank, const int* __restrict__ live, int p,
                                                                   double* __restrict__ rmat)
{
    const long long mat = blockIdx.y;
    if (!live[mat]) return;
    const int r = rank[mat];
    const long long it = (long long)blockIdx.x * EIGW_THREADS + threadIdx.x;
    if (it >= (long long)r * r) return;
    const int j = (int)(it / r), l = (int)(it - (long long)j * r);
    if (j > l) return;
    const cplx* __restrict__ Lm = reinterpret_cast<const cplx*>(L) + mat * p * p;
    const cplx* __restrict__ Tm = reinterpret_cast<const cplx*>(T) + mat * p * p;
    cplx a{0.0, 0.0}, b{0.0, 0.0};
    for (int i = 0; i < p; ++i) {
        const cplx lj = Lm[(long long)i * p + j], ll = Lm[(long long)i * p + l], tj = Tm[(long long)i * p + j], tl = Tm[(long long)i * p + l];
        a.re += lj.re * tl.re + lj.im * tl.im;  a.im += lj.re * tl.im - lj.im * tl.re;       // conj(L_ij) T_il
        b.re += ll.re * tj.re + ll.im * tj.im;  b.im += ll.re * tj.im - ll.im * tj.re;       // conj(L_il) T_ij
    }
    reinterpret_cast<cplx*>(rmat)[mat * p * p + (long long)j * p + l] = cplx{0.5 * (a.re + b.re), j == l ? 0.0 : 0.5 * (a.im - b.im)};
}

__global__ __launch_bounds__(EIGW_THREADS) void eigw_gedmd_back_kernel(const double* __restrict__ L, const double* __restrict__ w2,
                                                                      const double* __restrict__ v2, const int* __restrict__ st2a,
                                                                      const int* __restrict__ st2b, const int* __restrict__ rank, int nev, int p,
                                                                      double* __restrict__ ev, double* __restrict__ vec)
{
    const int tid = threadIdx.x;
    const long long mat = blockIdx.x;
    const int r = rank[mat], st = st2a[mat] + st2b[mat];
    if (r < nev || r > p || st == 0 || st > EIG_MAX_SWEEPS) return;           // the host refuses the call
    const double nan = __builtin_nan("");
    for (int k = tid; k < nev; k += EIGW_THREADS) ev[mat * nev + k] = st < 0 ? nan : w2[mat * p + r - nev + k];
    if (!vec) return;
    const cplx* __restrict__ Lm = reinterpret_cast<const cplx*>(L) + mat * p * p;
    const cplx* __restrict__ vm = reinterpret_cast<const cplx*>(v2) + mat * p * p;
    cplx* __restrict__ out = reinterpret_cast<cplx*>(vec) + mat * p * nev;
    for (int it = tid; it < p * nev; it += EIGW_THREADS) {
        const int i = it / nev, j = it - i * nev;
        cplx acc{nan, nan};
        if (st > 0) {
            acc = cplx{0.0, 0.0};
            for (int k = 0; k < r; ++k) {
                const cplx l = Lm[(long long)i * p + k], x = vm[(long long)k * p + (r - nev + j)];
                acc.re += l.re * x.re - l.im * x.im;
                acc.im += l.re * x.im + l.im * x.re;
            }
        }
        out[it] = acc;
    }
}

constexpr size_t EIGW_PAIR_LDS = 2 * (size_t)EIGW_PAIR * EIGW_PAIR * sizeof(cplx);      // 128 KiB: the pair's A and V, or U and a tile

}  // namespace

hipError_t launch_eigw_init(const EigWide& e, const double* a, long long mat_stride, int lda, hipStream_t st)
{
    hipLaunchKernelGGL(eigw_init_kernel, dim3((unsigned)e.n_mat), dim3(EIGW_THREADS), 0, st, e, a, mat_stride, lda);
    return hipGetLastError();
}

hipError_t launch_eigw_round(const EigWide& e, int r, hipStream_t st)
{
    // more than 64 KiB of dynamic LDS has to be asked for
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(eigw_pair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)EIGW_PAIR_LDS);
    if (err != hipSuccess) return err;
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(eigw_update_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)EIGW_PAIR_LDS);
    if (err != hipSuccess) return err;
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(eigw_update_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)EIGW_PAIR_LDS);
    if (err != hipSuccess) return err;
    const unsigned nslot = (unsigned)(eigw_slots(e.n) / 2), ntile = (unsigned)((e.n + EIGW_PAIR - 1) / EIGW_PAIR), nm = (unsigned)e.n_mat;
    hipLaunchKernelGGL(eigw_pair_kernel, dim3(nslot, nm), dim3(EIGW_PAIR_THREADS), EIGW_PAIR_LDS, st, e, r);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(eigw_update_kernel<false>, dim3(2 * ntile, nslot, nm), dim3(EIGW_THREADS), EIGW_PAIR_LDS, st, e, r, (int)ntile);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(eigw_update_kernel<true>, dim3(ntile, nslot, nm), dim3(EIGW_THREADS), EIGW_PAIR_LDS, st, e, r, (int)ntile);
    return hipGetLastError();
}

hipError_t launch_eigw_sweep_end(const EigWide& e, int sweep, hipStream_t st)
{
    hipLaunchKernelGGL(eigw_sweep_end_kernel, dim3((unsigned)((e.n_mat + 255) / 256)), dim3(256), 0, st, e, sweep);
    return hipGetLastError();
}

hipError_t launch_eigw_finish(const EigWide& e, double* w, double* v, int ldo, hipStream_t st)
{
    hipLaunchKernelGGL(eigw_finish_kernel, dim3((unsigned)e.n_mat), dim3(EIGW_THREADS), 0, st, e, w, v, ldo);
    return hipGetLastError();
}

hipError_t launch_eigw_gedmd_rank(const double* w1, const double* u1, const int* status1, double tol, int nev, int p, double* s, double* L,
                                  double* rmat, int* rank, int* nv_narrow, int* nv_wide, int* live, long long n_mat, hipStream_t st)
{
    hipLaunchKernelGGL(eigw_gedmd_rank_kernel, dim3((unsigned)n_mat), dim3(EIGW_THREADS), 0, st, w1, u1, status1, tol, nev, p, s, L, rmat, rank,
                       nv_narrow, nv_wide, live);
    return hipGetLastError();
}

hipError_t launch_eigw_gedmd_reduce(const double* gram, const double* kmat, double coef, const double* L, const int* rank, const int* live,
                                    int p, double* T, double* rmat, long long n_mat, hipStream_t st)
{
    const unsigned nblk = (unsigned)(((long long)p * p + EIGW_THREADS - 1) / EIGW_THREADS);
    hipLaunchKernelGGL(eigw_gedmd_t_kernel, dim3(nblk, (unsigned)n_mat), dim3(EIGW_THREADS), 0, st, gram, kmat, coef, L, rank, live, p, T);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(eigw_gedmd_r_kernel, dim3(nblk, (unsigned)n_mat), dim3(EIGW_THREADS), 0, st, L, T, rank, live, p, rmat);
    return hipGetLastError();
}

hipError_t launch_eigw_gedmd_back(const double* L, const double* w2, const double* v2, const int* st2a, const int* st2b, const int* rank,
                                  int nev, int p, double* ev, double* vec, long long n_mat, hipStream_t st)
{
    hipLaunchKernelGGL(eigw_gedmd_back_kernel, dim3((unsigned)n_mat), dim3(EIGW_THREADS), 0, st, L, w2, v2, st2a, st2b, rank, nev, p, ev, vec);
    return hipGetLastError();
}

}  // namespace ti
