// ff_device.hpp -- the analytic forces of the force field of obs_ff_kernels.hip (include/ti_hip.h ti_obs_ff_forces), one wave per
// molecule, as device functions: ti_obs_ff_forces and the Langevin kernel (ti_obs_ff_langevin) call this one body, so the integrator
// runs the forces the forces entry point pins.  Everything is fp64 without contraction (the pragma below), so the arithmetic does not
// depend on the kernel the body is inlined into.
//
// Summation order of an atom's force component (no atomics; independent of wave, workgroup, trip and batch position):
//   1. the bonded tables in the order bonds, angles, torsions; a table in chunks of 64 terms, chunks ascending.  Lane l evaluates term
//      64 q + l of chunk q and writes the force on each of its slots to the wave's staging area [64][4][3]; the component then adds
//      the entries of its atom from the host-built incidence list of the chunk (below) -- ascending term, one running sum
//      across chunks and tables, starting from 0;
//   2. the pairs, atom-centred: lane 2 a + s walks the partners j of atom a in [0, h) (s = 0) or [h, A) (s = 1), h = (A + 1) / 2,
//      ascending, skipping j = a and the rows that are not FF_LIVE; the atom's pair force is slice 0 + slice 1;
//   3. component = (running bonded sum) + (pair force).
// The energy of the same pass: lane l adds the energies of terms l, l + 64, ... of a table (pairs: of its partners j > a) in that
// order, the lane sums go through wave_sum; the total is ((bond + angle) + torsion) + pair as in obs_ff_energy_kernel.
#pragma once

#include "ode_device.hpp"

namespace ti {

// ---- the incidence list (built by ti_obs_ff_set next to the term words) -----------------------------------------------------------
// For every chunk q (bond chunks, then angle chunks, then torsion chunks) and atom a: the (lane, slot) entries of the chunk's terms
// that touch a, ascending in the term index, one byte each (lane << 2 | slot).  Packed into 32-bit words: FF_INC_OFF_WORDS words of
// uint16 offsets [n_chunks * A + 1] into the byte list, then the bytes.
constexpr int FF_CHUNK = 64;
constexpr int FF_MAX_CHUNKS = (TI_FF_MAX_BONDS + 63) / 64 + (TI_FF_MAX_ANGLES + 63) / 64 + (TI_FF_MAX_TORSIONS + 63) / 64;
constexpr int FF_INC_OFF_WORDS = (FF_MAX_CHUNKS * FF_MAX_ATOMS + 1 + 1) / 2;
constexpr int FF_INC_MAX_ENTRIES = 2 * TI_FF_MAX_BONDS + 3 * TI_FF_MAX_ANGLES + 4 * TI_FF_MAX_TORSIONS;
constexpr int FF_INC_WORDS = FF_INC_OFF_WORDS + (FF_INC_MAX_ENTRIES + 3) / 4;
constexpr int FF_STAGE_DOUBLES = FF_CHUNK * 4 * 3;
__host__ __device__ inline int ff_chunks(int n) { return (n + FF_CHUNK - 1) / FF_CHUNK; }

namespace {

constexpr int FFD_IDX_WORDS = TI_FF_MAX_BONDS + TI_FF_MAX_ANGLES + TI_FF_MAX_TORSIONS + TI_FF_MAX_PAIRS;
constexpr int FFD_PAR_DOUBLES = 2 * TI_FF_MAX_BONDS + 2 * TI_FF_MAX_ANGLES + 2 * TI_FF_MAX_TORSIONS + 3 * TI_FF_MAX_PAIRS;
constexpr int FFD_X_DOUBLES = 3 * FF_MAX_ATOMS + 1;

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 ld3(const double* s, int a) { return V3{s[3 * a], s[3 * a + 1], s[3 * a + 2]}; }
__device__ __forceinline__ void st3(double* s, V3 v) { s[0] = v.x; s[1] = v.y; s[2] = v.z; }

// the tables of a workgroup in LDS
struct FfView {
    const int32_t *wb, *wa, *wt, *wp;
    const double *pb, *pa, *pt, *pp;
    const uint16_t* inc_off; const uint8_t* inc;
    int nb, na, nt, np, A;
    double coulomb;
};

// LDS writes of one lane read by another lane of the same wave: the wave's LDS operations complete in order, the fence keeps the
// compiler from moving them
__device__ __forceinline__ void ff_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- per-term gradients: the energy of the term; g [slots][3] = the force on each slot ------------------------------------------
__device__ __forceinline__ double ff_bond_term(const double* sx, int32_t w, double r0, double k, double* g)
{
#pragma clang fp contract(off)
    const V3 a = ld3(sx, ff_atom(w, 0)), b = ld3(sx, ff_atom(w, 1));
    const V3 d{b.x - a.x, b.y - a.y, b.z - a.z};
    const double r = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z), dr = r - r0;
    const double c = -(k * dr) / r;                         // on slot 1: -k (r - r0) d / r
    st3(g + 3, V3{c * d.x, c * d.y, c * d.z});
    st3(g, V3{-(c * d.x), -(c * d.y), -(c * d.z)});
    return k * dr * dr * 0.5;
}

__device__ __forceinline__ double ff_angle_term(const double* sx, int32_t w, double th0, double k, double* g)
{
#pragma clang fp contract(off)
    const V3 c = ld3(sx, ff_atom(w, 1)), pi = ld3(sx, ff_atom(w, 0)), pk = ld3(sx, ff_atom(w, 2));
    const V3 u{pi.x - c.x, pi.y - c.y, pi.z - c.z}, v{pk.x - c.x, pk.y - c.y, pk.z - c.z};
    const double nu = sqrt((u.x * u.x + u.y * u.y) + u.z * u.z), nv = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
    double cs = ((u.x * v.x + u.y * v.y) + u.z * v.z) / (nu * nv);
    cs = cs > 1.0 ? 1.0 : cs < -1.0 ? -1.0 : cs;            // the energy kernel's clamp; a NaN stays a NaN
    const double dth = acos(cs) - th0;
    const double wgt = k * dth / sqrt((1.0 - cs) * (1.0 + cs));          // -dE / d cos = k (theta - theta0) / sin theta
    const V3 eu{u.x / nu, u.y / nu, u.z / nu}, ev{v.x / nv, v.y / nv, v.z / nv};
    const double wi = wgt / nu, wk = wgt / nv;
    const V3 gi{wi * (ev.x - cs * eu.x), wi * (ev.y - cs * eu.y), wi * (ev.z - cs * eu.z)};
    const V3 gk{wk * (eu.x - cs * ev.x), wk * (eu.y - cs * ev.y), wk * (eu.z - cs * ev.z)};
    st3(g, gi); st3(g + 6, gk);
    st3(g + 3, V3{-(gi.x + gk.x), -(gi.y + gk.y), -(gi.z + gk.z)});
    return k * dth * dth * 0.5;
}

// d phi / dx in the Blondel-Karplus form: no division by sin phi; singular only for collinear b1, b2 (m = 0) or b2, b3 (n = 0)
__device__ __forceinline__ double ff_torsion_term(const double* sx, int32_t w, double phase, double k, double* g)
{
#pragma clang fp contract(off)
    const V3 x1 = ld3(sx, ff_atom(w, 0)), x2 = ld3(sx, ff_atom(w, 1)), x3 = ld3(sx, ff_atom(w, 2)), x4 = ld3(sx, ff_atom(w, 3));
    const V3 b1{x2.x - x1.x, x2.y - x1.y, x2.z - x1.z}, b2{x3.x - x2.x, x3.y - x2.y, x3.z - x2.z}, b3{x4.x - x3.x, x4.y - x3.y, x4.z - x3.z};
    const V3 m{b1.y * b2.z - b1.z * b2.y, b1.z * b2.x - b1.x * b2.z, b1.x * b2.y - b1.y * b2.x};
    const V3 n{b2.y * b3.z - b2.z * b3.y, b2.z * b3.x - b2.x * b3.z, b2.x * b3.y - b2.y * b3.x};
    const double l2 = (b2.x * b2.x + b2.y * b2.y) + b2.z * b2.z, l = sqrt(l2);
    const double phi = atan2(l * ((b1.x * n.x + b1.y * n.y) + b1.z * n.z), (m.x * n.x + m.y * n.y) + m.z * n.z);
    const double per = (double)ff_period(w), arg = per * phi - phase;
    const double wgt = k * per * sin(arg);                  // -dE / d phi
    const double c1 = -l / ((m.x * m.x + m.y * m.y) + m.z * m.z), c4 = l / ((n.x * n.x + n.y * n.y) + n.z * n.z);
    const V3 d1{c1 * m.x, c1 * m.y, c1 * m.z}, d4{c4 * n.x, c4 * n.y, c4 * n.z};
    const double s12 = ((b1.x * b2.x + b1.y * b2.y) + b1.z * b2.z) / l2, s32 = ((b3.x * b2.x + b3.y * b2.y) + b3.z * b2.z) / l2;
    const V3 d2{(-d1.x - s12 * d1.x) + s32 * d4.x, (-d1.y - s12 * d1.y) + s32 * d4.y, (-d1.z - s12 * d1.z) + s32 * d4.z};
    const V3 d3{(-d4.x + s12 * d1.x) - s32 * d4.x, (-d4.y + s12 * d1.y) - s32 * d4.y, (-d4.z + s12 * d1.z) - s32 * d4.z};
    st3(g, V3{wgt * d1.x, wgt * d1.y, wgt * d1.z});
    st3(g + 3, V3{wgt * d2.x, wgt * d2.y, wgt * d2.z});
    st3(g + 6, V3{wgt * d3.x, wgt * d3.y, wgt * d3.z});
    st3(g + 9, V3{wgt * d4.x, wgt * d4.y, wgt * d4.z});
    return k * (1.0 + cos(arg));
}

// the pair (a, j): f += the force on a; returns the pair's energy (the energy kernel's expression)
__device__ __forceinline__ double ff_pair_term(const double* sx, int a, int j, double qq, double sigma, double eps, double coulomb, V3& f)
{
#pragma clang fp contract(off)
    const V3 pa = ld3(sx, a), pj = ld3(sx, j);
    const V3 d{pa.x - pj.x, pa.y - pj.y, pa.z - pj.z};
    const double r2 = (d.x * d.x + d.y * d.y) + d.z * d.z, r = sqrt(r2);
    double lj = 0.0, cl = 0.0, c = 0.0;
    if (eps > 0.0 && sigma > 0.0) {
        const double q = sigma / r, q2 = q * q, s6 = q2 * q2 * q2;
        lj = 4.0 * eps * s6 * (s6 - 1.0);
        c = 24.0 * eps * s6 * (2.0 * s6 - 1.0) / r2;
    }
    if (qq != 0.0) {
        cl = coulomb * qq / r;
        c = c + coulomb * qq / (r2 * r);
    }
    f.x = f.x + c * d.x; f.y = f.y + c * d.y; f.z = f.z + c * d.z;
    return (lj == HUGE_VAL) ? lj : lj + cl;                 // r = 0: the wall wins over an attractive charge product
}

// one bonded table: n terms from chunk number q0 on; acc0 / acc1 = the running sums of components lane and lane + 64
template <int SLOTS>
__device__ __forceinline__ double ff_bonded_table(const FfView& t, const int32_t* words, const double* par, int n, int q0, const double* sx,
                                                  double* stage, int lane, double& acc0, double& acc1)
{
#pragma clang fp contract(off)
    double e = 0.0;
    const int m3 = 3 * t.A;
    for (int base = 0, q = q0; base < n; base += FF_CHUNK, ++q) {
        const int term = base + lane;
        if (term < n) {
            const int32_t w = words[term];
            double* g = stage + lane * 12;
            if (SLOTS == 2) e = e + ff_bond_term(sx, w, par[2 * term], par[2 * term + 1], g);
            else if (SLOTS == 3) e = e + ff_angle_term(sx, w, par[2 * term], par[2 * term + 1], g);
            else e = e + ff_torsion_term(sx, w, par[2 * term], par[2 * term + 1], g);
        }
        ff_wave_sync();
        for (int half = 0; half < 2; ++half) {
            const int c = lane + 64 * half;
            if (c >= m3) break;
            const int a = c / 3, k = c - 3 * a;
            double s = half ? acc1 : acc0;
            for (int i = t.inc_off[q * t.A + a], end = t.inc_off[q * t.A + a + 1]; i < end; ++i) {
                const int en = t.inc[i];
                s = s + stage[(en >> 2) * 12 + (en & 3) * 3 + k];
            }
            if (half) acc1 = s; else acc0 = s;
        }
        ff_wave_sync();                                     // the next chunk overwrites the staging area
    }
    return e;
}

// The forces of the wave's molecule at sx [3A] (fp64 nm, LDS) into sf [3A] (LDS), through the wave's staging area (FF_STAGE_DOUBLES,
// LDS); e[4] = the bond, angle, torsion and pair energies (the same bits in every lane).  sx must be visible to the wave on entry;
// sf is visible to it on return.
__device__ __forceinline__ void ff_wave_forces(const FfView& t, const double* sx, double* sf, double* stage, int lane, double (&e)[4])
{
#pragma clang fp contract(off)
    double acc0 = 0.0, acc1 = 0.0;
    const int qa = ff_chunks(t.nb), qt = qa + ff_chunks(t.na);
    double eb = ff_bonded_table<2>(t, t.wb, t.pb, t.nb, 0, sx, stage, lane, acc0, acc1);
    double ea = ff_bonded_table<3>(t, t.wa, t.pa, t.na, qa, sx, stage, lane, acc0, acc1);
    double et = ff_bonded_table<4>(t, t.wt, t.pt, t.nt, qt, sx, stage, lane, acc0, acc1);
    double ep = 0.0;
    const int A = t.A, a = lane >> 1, s = lane & 1, h = (A + 1) / 2;
    V3 f{0.0, 0.0, 0.0};
    if (a < A) {
        for (int j = s ? h : 0, end = s ? A : h; j < end; ++j) {
            if (j == a) continue;
            const int lo = a < j ? a : j, hi = a < j ? j : a;
            const int row = lo * (2 * A - lo - 1) / 2 + (hi - lo - 1);
            if (!(t.wp[row] & FF_LIVE)) continue;
            const double pe = ff_pair_term(sx, a, j, t.pp[3 * row], t.pp[3 * row + 1], t.pp[3 * row + 2], t.coulomb, f);
            if (j > a) ep = ep + pe;
        }
    }
    f.x = f.x + __shfl_xor(f.x, 1); f.y = f.y + __shfl_xor(f.y, 1); f.z = f.z + __shfl_xor(f.z, 1);       // slice 0 + slice 1
    if (a < A && s == 0) st3(stage + 3 * a, f);
    ff_wave_sync();
    if (lane < 3 * A) sf[lane] = acc0 + stage[lane];
    if (lane + 64 < 3 * A) sf[lane + 64] = acc1 + stage[lane + 64];
    ff_wave_sync();
    e[0] = wave_sum(eb); e[1] = wave_sum(ea); e[2] = wave_sum(et); e[3] = wave_sum(ep);
}

}  // namespace

}  // namespace ti
