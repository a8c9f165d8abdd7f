// painn_pair_kernel_body.inc -- the body of the pair-major message kernel (painn_pair_kernel.hpp), included once for painn_pair_kernel
// and once for its masked twin painn_pair_mask_kernel, and once for painn_pair_general_kernel (TI_PAIR_GENERAL).  TI_PAIR_ROWS: the wave's row words -- the template's in the first; its own
// group's in the second, whose per-group row words mark pairs absent from their molecule invalid (w factor 0, like missing pairs).
// GENERAL: the build that walks the template's general blocks [n_tile, nblk) -- 16 unrelated pairs, no slots -- after the tile build
// has walked [0, n_tile) (pair_template.hpp).  Everything up to the output products is per row and shared; the output stage then adds
// every row's contributions of both directions to the row's own two atoms instead of forming slot sums.
// TI_PAIR_SEEDED: the seeded twins (painn_pair_seeded_kernel, painn_pair_general_seeded_kernel): general rows store, tile slots only add.
{
    static_assert(PREC == 0 || PREC == 1, "the fp16 storage mode keeps the directed message kernel");
    static_assert(!TABLE || (FIRST && PREC == 1), "the phi table serves layer 0 of the split path");
    constexpr bool GENERAL = TI_PAIR_GENERAL;
    static_assert(!GENERAL || pair_general_build_exists(PREC), "general blocks: the split path, which folds the cross term (the f32 path keeps the tile-only template)");
    // SEEDED (a seeded template, pair_template.hpp; plain split-path batches): the general launch runs first and every valid general row
    // is its two atoms' first contribution of the layer -- GENERAL && SEEDED writes dsacc / dvacc with plain stores, no atomic and no
    // read; the tile launch after it (!GENERAL && SEEDED) finds every accumulator row seeded and only adds: no first touch
    constexpr bool SEEDED = TI_PAIR_SEEDED;
    static_assert(!SEEDED || pair_general_build_exists(PREC), "seeded accumulators: the split path, whose templates have general blocks");
    // TAILS (painn_pair_general_tails_kernel: GENERAL && SEEDED on a template with merged tails, pair_template.hpp): one wave owns a
    // SUPER-GROUP of S = p.tail_S groups.  It walks the full general blocks [n_tile, nblk - 1) of each of them as the seeded general
    // build does, then ONE merged block for the S last blocks, which hold r = p.tail_r = 16 / S valid rows each: merged row j is row
    // j % r of the last block of group j / r.  The owning group is then per lane -- j / r in the row layout, (4q) / r in the flipped
    // one (r is a multiple of 4: the four rows of a lane row belong to one group) -- and so is everything derived from it.  A row's
    // value does not depend on its block mates, every row keeps its storage, so the results are those of the unmerged walk bit for bit.
    constexpr bool TAILS = TI_PAIR_TAILS;
    static_assert(!TAILS || (GENERAL && SEEDED), "merged tails: the seeded general launch");
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, T = 64 * WAVES, CH4 = edge_chunk4(NB, false);
    using A16 = r16::Act<NBK>;
    constexpr bool ONE = edge_one_chain(PREC);
    using OP = std::conditional_t<ONE, r16::Opnd1<NBK>, typename r16::OpSel<NBK, PREC>::type>;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    constexpr int SC = pair_superchunk(NB, WAVES, TABLE), NBUF = 2;                 // two superchunks in LDS (PipeDMA)
    const int blk_lo = GENERAL ? p.n_tile : 0, blk_hi = GENERAL ? p.nblk : p.n_tile;
    float* scratch = reinterpret_cast<float*>(lds + NBUF * SC * CH4) + wave * 64;  // [16 pair rows][4] edge_dir of direction A
    float* vec = reinterpret_cast<float*>(lds + NBUF * SC * CH4) + WAVES * 64;     // [EV::COUNT][F]
    for (int i = threadIdx.x; i < EV::COUNT * F / 4; i += T)
        reinterpret_cast<f32x4*>(vec)[i] = reinterpret_cast<const f32x4*>(p.vecs)[i];
    PipeDMA<NB, T, SC, CH4> pipe;        // two buffers, one closing barrier per superchunk (mfma_chain.hpp)
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);

    const float eps_w0 = ONE ? 1e-5f * p.wscale[0] * p.wscale[0] : 1e-5f, eps_w1 = ONE ? 1e-5f * p.wscale[1] * p.wscale[1] : 1e-5f;
    const float eps_p0 = ONE ? 1e-5f * p.wscale[2] * p.wscale[2] : 1e-5f, eps_p1 = ONE ? 1e-5f * p.wscale[3] * p.wscale[3] : 1e-5f;
    const float s_p0 = ONE ? p.wscale[2] : 1.0f, inv_out = ONE ? 1.0f / (p.wscale[4] * p.wscale[5]) : 1.0f;
    const long long gi_raw = (long long)blockIdx.x * WAVES + wave;                // TAILS: the wave's super-group, gi its first group
    const bool group_ok = (TAILS ? gi_raw * p.tail_S : gi_raw) < p.n_groups;
    const long long gi = group_ok ? (TAILS ? gi_raw * p.tail_S : gi_raw) : p.n_groups - 1;
    // The group's first node is the same for the whole wave, so the node arrays are addressed from per-group bases that live in scalar
    // registers, with the node inside the group (< G * A) as an unsigned 32-bit lane offset: the 64-bit part of every address is scalar
    // work (DESIGN.md 3.6)
    const long long gnode0 = gi * p.G * (long long)p.A;
    const unsigned mol_cap = (unsigned)(p.B - 1 - gi * p.G);               // molecules past the batch's end read the last one
    auto lnode_of = [&](int mol_local, int atom) {
        const unsigned m = (unsigned)mol_local < mol_cap ? (unsigned)mol_local : mol_cap;
        return m * (unsigned)p.A + (unsigned)atom;
    };
    const float* const x_g = p.x + gnode0 * 3;
    const float* const P_g = p.P + gnode0 * F;
    const float* const v_g = p.v + gnode0 * 3 * F;
    float* const ds_g = p.dsacc + gnode0 * F;
    float* const dv_g = p.dvacc + gnode0 * 3 * F;
    float* const c_g = p.cacc + gnode0 * 3 * F;
    // TABLE: the classes of the group's molecules, four bits each, in one scalar word (molecules past the batch's end: the last one's),
    // and from them the offset of a (molecule in group, atom, edge type) row of the phi table
    unsigned clsw = 0;
    if constexpr (TABLE && !TAILS)
        for (int m = 0; m < p.G; ++m) clsw |= (unsigned)p.cls[gi * p.G + ((unsigned)m < mol_cap ? (unsigned)m : mol_cap)] << (4 * m);
    auto tab_off = [&](int mol_local, int atom, int type) {
        const unsigned cls = (clsw >> (4 * mol_local)) & 15u;
        return ((cls * (unsigned)p.A + (unsigned)atom) * (unsigned)PHI0_TYPES + (unsigned)type) * (unsigned)(3 * F);
    };
    auto tab_off_of = [&](unsigned word, int mol_local, int atom, int type) {      // TAILS: the class word is the lane's group's
        const unsigned cls = (word >> (4 * mol_local)) & 15u;
        return ((cls * (unsigned)p.A + (unsigned)atom) * (unsigned)PHI0_TYPES + (unsigned)type) * (unsigned)(3 * F);
    };

    // Diagnostic build only (-DTI_STAMPS; never the product): shader-clock stamps of ONE row block of a few workgroups, and one
    // (s_memtime, s_memrealtime) pair around the whole block loop of every wave for the in-kernel clock (MI355X guide, DVFS item 6).
    // Stamps go to a buffer of their own that nothing else reads.
#ifdef TI_STAMPS
    constexpr int STAMP_SLOTS = 64;
    const bool st_wg = blockIdx.x >= 300 && blockIdx.x < 304;
    unsigned long long* const st_buf = p.stamps ? p.stamps + ((size_t)(blockIdx.x - 300) * WAVES + wave) * STAMP_SLOTS : nullptr;
    int st_i = 0;
    unsigned long long clk0 = 0, rt0 = 0;
    if (p.stamps) { clk0 = __builtin_amdgcn_s_memtime(); rt0 = __builtin_amdgcn_s_memrealtime(); }
#define TI_STAMP() do { if (st_wg && st_buf && blk == 3 && st_i < STAMP_SLOTS) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) st_buf[st_i] = t_; ++st_i; } } while (0)
#else
#define TI_STAMP() do { } while (0)
#endif

    // TAILS: the walk is S * (full general blocks) + 1 steps, the same for every wave of the workgroup (they share the weight ring);
    // step `it` is block n_tile + it % n_full of group gi + it / n_full, the last step the merged block (stored as block nblk - 1)
    const int n_full = TAILS ? p.nblk - 1 - p.n_tile : 1, n_walk = TAILS ? p.tail_S * n_full + 1 : 0;
    const int tail_sh = TAILS ? __builtin_ctz((unsigned)p.tail_r) : 0;            // r is a power of two
    auto walk_blk = [&](int it) { return it == n_walk - 1 ? p.nblk - 1 : p.n_tile + it % n_full; };
    for (int blk = TAILS ? walk_blk(0) : blk_lo, it = 0; TAILS ? it < n_walk : blk < blk_hi; TAILS ? (void)(++it, blk = walk_blk(it)) : (void)++blk) {
        TI_STAMP();
        // TAILS: who owns the rows of this step.  gi is the super-group's FIRST group and every per-group base above stays a scalar; the
        // lane's group is gi + subR in the row layout (lane (j, q): row j) and gi + subF in the flipped one (rows 4q + r), and reaches
        // the node arrays, the class map and the row storage (rsub rows on) as a 32-bit lane offset from those bases.  okR / okF: that
        // group exists.  rowj / frow0: the rows' places in their block's storage.  Every other build: the wave's group, rows j, 4q + r.
        int subR = 0, subF = 0, rowj = 0, frow0 = 0;
        bool okR = false, okF = false;
        unsigned rsub = 0, erow_l = 0, clswR = 0, clswF = 0;
        if constexpr (TAILS) {
            const bool merged = it == n_walk - 1;
            subR = merged ? j >> tail_sh : it / n_full; subF = merged ? (4 * q) >> tail_sh : it / n_full;
            okR = group_ok && gi + subR < p.n_groups; okF = group_ok && gi + subF < p.n_groups;
            if (!okR) subR = 0;
            if (!okF) subF = 0;
            rowj = merged ? j & (p.tail_r - 1) : j; frow0 = merged ? (4 * q) & (p.tail_r - 1) : 4 * q;
            rsub = (unsigned)(subR * p.nblk * 16);
            erow_l = (2u * rsub + (unsigned)rowj) * (unsigned)F;             // the lane's e row from erowA / erowB
            if constexpr (TABLE)
                for (int m = 0; m < p.G; ++m) {
                    const unsigned mR = (unsigned)(subR * p.G + m), mF = (unsigned)(subF * p.G + m);
                    clswR |= (unsigned)p.cls[gi * p.G + (mR < mol_cap ? mR : mol_cap)] << (4 * m);
                    clswF |= (unsigned)p.cls[gi * p.G + (mF < mol_cap ? mF : mol_cap)] << (4 * m);
                }
        }
        auto lnode_r = [&](int mol_local, int atom) { return lnode_of(subR * p.G + mol_local, atom); };
        auto lnode_f = [&](int mol_local, int atom) { return lnode_of(subF * p.G + mol_local, atom); };
        // ---- K1 geometry of this lane's pair row (the 4 quarters compute the same row); direction A: r = x[I] - x[J]
        const uint32_t meta = TI_PAIR_ROWS[blk * 16 + (TAILS ? rowj : j)];
        const unsigned lI = TAILS ? lnode_r(prow_molI(meta), prow_atomI(meta)) : lnode_of(prow_molI(meta), prow_atomI(meta)), lJ = TAILS ? lnode_r(prow_molJ(meta), prow_atomJ(meta)) : lnode_of(prow_molJ(meta), prow_atomJ(meta));   // the row's two nodes inside the group
        // row_ok: this lane's pair row exists.  A row that does not contributes nothing (w factor 0) and no valid row reads its e row,
        // its parked encoding or its edge_dir: it loads none of them (zeros instead) and stores none
        // (TAILS: nor does a row of a group past the batch's end)
        const bool row_ok = TAILS ? (meta & 1u) != 0 && okR : (meta & 1u) != 0;
        const size_t brow0 = ((size_t)gi * p.nblk + blk) * 16;       // pair rows: parked encoding / edge_dir
        const size_t erowA = brow0 * 2, erowB = erowA + 16;             // e rows of the two directions
        OP enc;
        f32x4* const enc_park = TAILS ? reinterpret_cast<f32x4*>(p.enc) + (brow0 / 16) * (sizeof(OP) / 16) * 64 + ((rsub / 16) * (unsigned)(sizeof(OP) / 16 * 64) + (unsigned)(16 * q + rowj))
                                      : reinterpret_cast<f32x4*>(p.enc) + (brow0 / 16) * (sizeof(OP) / 16) * 64 + lane;
        f32x4* const geo_park = TAILS ? reinterpret_cast<f32x4*>(p.geo) + brow0 + (rsub + (unsigned)rowj) : reinterpret_cast<f32x4*>(p.geo) + brow0 + j;
        if constexpr (FIRST) {
            const float* const xI = x_g + lI * 3u;
            const float* const xJ = x_g + lJ * 3u;
            const float rx = xI[0] - xJ[0];
            const float ry = xI[1] - xJ[1];
            const float rz = xI[2] - xJ[2];
            const float dist = sqrtf(rx * rx + ry * ry + rz * rz);
            const float den = 1.0f + dist;                       // edge_dir = r / (1 + d)   (not a unit vector)
            if (q == 0) {
                f32x4 dd = {rx / den, ry / den, rz / den, 0.f};
                *reinterpret_cast<f32x4*>(scratch + j * 4) = dd;
                if ((TAILS ? okR : group_ok) && row_ok) *geo_park = dd;
            }
            A16 t;
            r16::posenc_set(t, dist / p.length_scale, q);
            enc.set(t);
            if ((TAILS ? okR : group_ok) && row_ok) r16::opnd_store(enc, enc_park);
        } else {
            if (q == 0) {
                f32x4 dd = {0.f, 0.f, 0.f, 0.f};
                if (row_ok) dd = *geo_park;
                *reinterpret_cast<f32x4*>(scratch + j * 4) = dd;
            }
            __builtin_memset(&enc, 0, sizeof(OP));
            if (row_ok) r16::opnd_load(enc, enc_park);
        }
        TI_STAMP();
        // ---- w(enc(d)) hidden layers, once per pair
        OP g2;
        {
            OP g1;
            A16 t1;
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                f32x4 a0 = r16::load_block(vec + EV::W_B0 * F, 2 * c, q), a1 = r16::load_block(vec + EV::W_B0 * F, 2 * c + 1, q);
                r16::gemm_on_pipe<false>(a0, a1, enc, pipe, lane);
                t1.b[2 * c] = a0; t1.b[2 * c + 1] = a1;
                pipe.release();
            }
            TI_STAMP();
            r16::ln_silu(t1, vec + EV::W_G0 * F, vec + EV::W_BE0 * F, q, eps_w0);
            g1.set(t1);
            TI_STAMP();
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                f32x4 a0 = r16::load_block(vec + EV::W_B1 * F, 2 * c, q), a1 = r16::load_block(vec + EV::W_B1 * F, 2 * c + 1, q);
                r16::gemm_on_pipe<false>(a0, a1, g1, pipe, lane);
                t1.b[2 * c] = a0; t1.b[2 * c + 1] = a1;
                pipe.release();
            }
            TI_STAMP();
            r16::ln_silu(t1, vec + EV::W_G1 * F, vec + EV::W_BE1 * F, q, eps_w1);
            g2.set(t1);
            TI_STAMP();
        }
        // ---- phi([s[src] | e]) hidden layers of both directions in lock step; the s[src] half of the first Linear is P[src]
        OP h2A, h2B;                                     // (TABLE: never set, never read)
        if constexpr (!TABLE) {
            OP inA, inB;
            A16 tA, tB;
            float scA, scB;
            if (FIRST) {
                r16::load_set(tA, p.edge_emb + prow_type(meta) * F, q);      // e = edge_emb[type], the same row for both directions
                scA = inA.set_scaled(tA);
                inB = inA; scB = scA;
            } else {
#pragma unroll
                for (int nb = 0; nb < NBK; ++nb) { tA.b[nb] = f32x4{0.f, 0.f, 0.f, 0.f}; tB.b[nb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
                if (row_ok) {
                    r16::load_set(tA, p.e + erowA * F + (TAILS ? erow_l : (unsigned)(j * F)), q);
                    r16::load_set(tB, p.e + erowB * F + (TAILS ? erow_l : (unsigned)(j * F)), q);
                }
                scA = inA.set_scaled(tA);                                    // e is an un-normalised stream: per-row 2^k
                scB = inB.set_scaled(tB);
            }
            const float ivA = r16::pow2_inverse(scA) * s_p0, ivB = r16::pow2_inverse(scB) * s_p0;
            TI_STAMP();
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const float* const PI = P_g + lI * (unsigned)F;
                const float* const PJ = P_g + lJ * (unsigned)F;
                f32x4 a0 = r16::load_block(PI, 2 * c, q) * ivA, a1 = r16::load_block(PI, 2 * c + 1, q) * ivA;
                f32x4 b0 = r16::load_block(PJ, 2 * c, q) * ivB, b1 = r16::load_block(PJ, 2 * c + 1, q) * ivB;
                r16::gemm_x2_on_pipe<false>(a0, a1, b0, b1, inA, inB, pipe, lane);
                tA.b[2 * c] = a0 * scA; tA.b[2 * c + 1] = a1 * scA;
                tB.b[2 * c] = b0 * scB; tB.b[2 * c + 1] = b1 * scB;
                pipe.release();
            }
            TI_STAMP();
            r16::ln_silu(tA, vec + EV::P_G0 * F, vec + EV::P_BE0 * F, q, eps_p0);
            r16::ln_silu(tB, vec + EV::P_G0 * F, vec + EV::P_BE0 * F, q, eps_p0);
            inA.set(tA); inB.set(tB);
            TI_STAMP();
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                f32x4 a0 = r16::load_block(vec + EV::P_B1 * F, 2 * c, q), a1 = r16::load_block(vec + EV::P_B1 * F, 2 * c + 1, q);
                f32x4 b0 = a0, b1 = a1;
                r16::gemm_x2_on_pipe<false>(a0, a1, b0, b1, inA, inB, pipe, lane);
                tA.b[2 * c] = a0; tA.b[2 * c + 1] = a1;
                tB.b[2 * c] = b0; tB.b[2 * c + 1] = b1;
                pipe.release();
            }
            TI_STAMP();
            r16::ln_silu(tA, vec + EV::P_G1 * F, vec + EV::P_BE1 * F, q, eps_p1);
            r16::ln_silu(tB, vec + EV::P_G1 * F, vec + EV::P_BE1 * F, q, eps_p1);
            h2A.set(tA); h2B.set(tB);
            TI_STAMP();
        }
        // ---- output layer, flipped: features on lanes (l & 15), pair rows 4q + r in registers: I slot q, J slots r
        uint32_t mi[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) mi[r] = TI_PAIR_ROWS[blk * 16 + (TAILS ? frow0 + r : 4 * q + r)];
        f32x4 wfac;                                      // row mask x 1 / (S_phi S_w): rides on the shared w factor
#pragma unroll
        for (int r = 0; r < 4; ++r) wfac[r] = (mi[r] & 1u) ? inv_out : 0.0f;
        // the destination atoms of this lane row: direction A's sums belong to J slot q, direction B's to I slot q; molecules of the batch only
        const int snJ = p.slotnode[blk * 16 + 4 + q], snI = p.slotnode[blk * 16 + q];
        const bool haveA = group_ok && snJ >= 0 && gi * p.G + slot_mol(snJ) < p.B;
        const bool haveB = group_ok && snI >= 0 && gi * p.G + slot_mol(snI) < p.B;
        const bool qfA = !SEEDED && (snJ & SLOT_FIRST_TOUCH) != 0, qfB = !SEEDED && (snI & SLOT_FIRST_TOUCH) != 0;      // SEEDED: every put adds
        // their nodes inside the group; touched only where haveA / haveB hold
        const unsigned lnA = (unsigned)slot_mol(snJ) * (unsigned)p.A + (unsigned)(snJ & 255), lnB = (unsigned)slot_mol(snI) * (unsigned)p.A + (unsigned)(snI & 255);
        // the accumulator rows of a node, laid out as three arrays (ds [F], dv [3F], c [3F] per node); off: ds 0.., dv F.., c 4F..
        auto acc_ptr = [&](unsigned lnode, int off) {
            return off < F ? ds_g + (lnode * (unsigned)F + (unsigned)off) : off < 4 * F ? dv_g + (lnode * (unsigned)(3 * F) + (unsigned)(off - F)) : c_g + (lnode * (unsigned)(3 * F) + (unsigned)(off - 4 * F));
        };
        // GENERAL: the two atoms of each of the lane's four rows -- sources of directions A and B, each the other's destination -- and
        // whether the row adds anything: it exists (masked twin: in its molecule) and its molecule is one of the batch
        unsigned gI[4], gJ[4];
        bool gok[4];
        if constexpr (GENERAL) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (TAILS) {
                    gI[r] = lnode_f(prow_molI(mi[r]), prow_atomI(mi[r])); gJ[r] = lnode_f(prow_molJ(mi[r]), prow_atomJ(mi[r]));
                    gok[r] = okF && (mi[r] & 1u) != 0 && (gi + subF) * p.G + prow_molI(mi[r]) < p.B;
                } else {
                    gI[r] = lnode_of(prow_molI(mi[r]), prow_atomI(mi[r])); gJ[r] = lnode_of(prow_molJ(mi[r]), prow_atomJ(mi[r]));
                    gok[r] = group_ok && (mi[r] & 1u) != 0 && gi * p.G + prow_molI(mi[r]) < p.B;
                }
            }
        }
        // both directions of the lane's four rows: direction A's value goes to the row's J atom, direction B's to its I atom, plain adds
        // (a general row never carries first touch: both atoms own a slot of an earlier tile block).  SEEDED: plain stores -- the row is
        // the only one of this launch that names either atom, and the tile launch that adds to them starts after this one has ended
        auto row_out = [&](float* d, float z) {
            if constexpr (SEEDED) *d = z;
            else acc_out(d, z, false);
        };
        auto put_rows = [&](const f32x4& a0, const f32x4& a1, const f32x4& b0, const f32x4& b1, int off) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (gok[r]) {
                    float* dA = acc_ptr(gJ[r], off);
                    float* dB = acc_ptr(gI[r], off);
                    row_out(dA, a0[r]); row_out(dA + 16, a1[r]);
                    row_out(dB, b0[r]); row_out(dB + 16, b1[r]);
                }
        };
        const unsigned lIq = lnode_of(prow_molI(mi[0]), prow_atomI(mi[0]));      // source of direction A for all four rows of this lane
        // TABLE: the table rows of this lane's values.  Flipped layout: the four pair rows 4q + r, source I[q] for direction A and J[r]
        // for direction B (a loose block mixes molecules, hence classes, inside one lane: every row has its own offset); row layout
        // (the de slice): pair row j.  Rows that do not exist name an atom that does, so what they load is finite (their w factor is 0).
        unsigned tfA[4], tfB[4], trA = 0, trB = 0;
        f32x4 tv[3][4];                                  // this 32-feature block's table values: [ds | scale_edge_dir | de][A0, A1, B0, B1]
        if constexpr (TABLE) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                tfA[r] = (TAILS ? tab_off_of(clswF, prow_molI(mi[r]), prow_atomI(mi[r]), prow_type(mi[r])) : tab_off(prow_molI(mi[r]), prow_atomI(mi[r]), prow_type(mi[r]))) + (unsigned)j;
                tfB[r] = (TAILS ? tab_off_of(clswF, prow_molJ(mi[r]), prow_atomJ(mi[r]), prow_type(mi[r])) : tab_off(prow_molJ(mi[r]), prow_atomJ(mi[r]), prow_type(mi[r]))) + (unsigned)j;
            }
            trA = TAILS ? tab_off_of(clswR, prow_molI(meta), prow_atomI(meta), prow_type(meta)) : tab_off(prow_molI(meta), prow_atomI(meta), prow_type(meta));
            trB = TAILS ? tab_off_of(clswR, prow_molJ(meta), prow_atomJ(meta), prow_type(meta)) : tab_off(prow_molJ(meta), prow_atomJ(meta), prow_type(meta));
        }

        // (phi_c + b) of both directions times the shared (w_c + b) for output slice c (0 gates, 1 scale_edge_dir, 2 ds, 3 de,
        // 4 cross gates), features fo .. fo+31 as two 16-feature blocks
        auto out3 = [&](int c, int nbo, f32x4& rA0, f32x4& rA1, f32x4& rB0, f32x4& rB1) {
            const float* bp = vec + (EV::P_B2 + c) * F + 32 * nbo + j;
            const float* bw = vec + (EV::W_B2 + c) * F + 32 * nbo + j;
            // the bias is one scalar per lane here (features on lanes) and already carries the scale of its matrix (painn_pack.hip: the
            // message kernel's vector block), i.e. the scale the one-accumulator products carry: it seeds the sums, like the hidden
            // layers' and the de slice's
            const float p0 = bp[0], p1 = bp[16], q0 = bw[0], q1 = bw[16];
            f32x4 a0 = {p0, p0, p0, p0}, a1 = {p1, p1, p1, p1}, b0 = a0, b1 = a1, w0 = {q0, q0, q0, q0}, w1 = {q1, q1, q1, q1};
            if constexpr (TABLE) {
                const int sl = c == 2 ? 0 : 1;
                a0 = tv[sl][0]; a1 = tv[sl][1]; b0 = tv[sl][2]; b1 = tv[sl][3];
            } else {
                r16::gemm_x2_on_pipe<true>(a0, a1, b0, b1, h2A, h2B, pipe, lane);
                pipe.release();
            }
            r16::gemm_on_pipe<true>(w0, w1, g2, pipe, lane);
            pipe.release();
            w0 *= wfac; w1 *= wfac;
            rA0 = a0 * w0; rA1 = a1 * w1;
            rB0 = b0 * w0; rB1 = b1 * w1;
        };
        // direction A: sum over the four lane rows (the I slots) for each register (J slot); lane row q' ends with J slot q'
        auto sumA = [&](const f32x4& v) {
            using QS = r16::QuarterSum<4>;
            return QS::swap32_add(QS::swap16_add(v[0], v[1]), QS::swap16_add(v[2], v[3]));
        };
        // off: offset of the quantity inside a node's accumulator rows (ds 0, dv (1 + c) F, c (4 + c) F) plus the lane's feature
        auto putA = [&](float z0, float z1, int off) {
            if (haveA) { float* d = acc_ptr(lnA, off); acc_out(d, z0, qfA); acc_out(d + 16, z1, qfA); }
        };
        auto putB = [&](float z0, float z1, int off) {
            if (haveB) { float* d = acc_ptr(lnB, off); acc_out(d, z0, qfB); acc_out(d + 16, z1, qfB); }
        };
        // direction B: the four registers of a lane are the J slots of ONE destination I[q]
        auto sumB = [&](const f32x4& v) { return (v[0] + v[1]) + (v[2] + v[3]); };
        auto emitA = [&](const f32x4& v0, const f32x4& v1, int off) { putA(sumA(v0), sumA(v1), off); };
        auto emitB = [&](const f32x4& v0, const f32x4& v1, int off) { putB(sumB(v0), sumB(v1), off); };
        // the value of lane row r' in every lane row, r' = 0 .. 3 (VALU lane swaps, mfma_chain.hpp)
        auto rows4 = [&](float x, float (&o)[4]) {
            float a = x, b = x;
            lane_swap16(a, b);                       // a = [X0 X0 X2 X2], b = [X1 X1 X3 X3]
            o[0] = a; o[2] = a; lane_swap32(o[0], o[2]);
            o[1] = b; o[3] = b; lane_swap32(o[1], o[3]);
        };
        // v[src] rows of the equivariant slice.  Split path: every VMEM load of the slice is issued and consumed BEFORE its first accumulator
        // atomic, and direction B's four source atoms J[r] are fetched once, by lane row r, and handed round with lane swaps.  Loads and
        // writes share vmcnt but complete out of order with respect to each other, so waiting for a load while atomics are in flight
        // costs `s_waitcnt vmcnt(0)`, the drain of those atomics -- with the gathers between the slice's atomics (three rounds per 32
        // features) the launch took 29.60 ms, this way 28.23 (profiles/r03i_dv_reorder_timing.txt; the r03c stamps had shown the slice
        // at 11 - 13 k cycles against 3 - 5 k for the others).  The f32 path is bound by its matrix instructions and short of registers:
        // it keeps the gathers next to their use.
        constexpr bool GATHER_EARLY = PREC != 0;
        // the cross-gate slice folded into dv (pair_folds_cross, ti_internal.hpp): the split path, which holds v[dst] of both directions
        // in registers; layer 0 has no such slice.  The f32 path sums cg * dir into cacc for the update kernel to cross.
        constexpr bool FOLD = pair_folds_cross(PREC) && !FIRST;
        f32x4* const zpark = reinterpret_cast<f32x4*>(vec + EV::COUNT * F) + wave * (GENERAL ? 8 : 3) * 64 + lane;     // FOLD: [3][64 lanes] f32x4 per wave (GENERAL: [8])
        static_assert(!FOLD || GATHER_EARLY, "the fold crosses with the v[dst] rows that the early gathers hold");
        const unsigned lJq = snJ >= 0 ? lnode_of(slot_mol(snJ), snJ & 255) : lIq;   // J slot q's atom: lane row q fetches it for all four
        const float wrow = (meta & 1u) ? inv_out : 0.0f;                 // the same row factor in the row layout (lane (j, q): row j)

#pragma unroll 1
        for (int nbo = 0; nbo < NB; ++nbo) {
            const int fo = 32 * nbo + j;
            TI_STAMP();
            if constexpr (TABLE) {
                // every table value of this feature block, fetched ahead of the block's first w product: the table stays in L2
                const float* const tb = p.phi0_tab + 32 * nbo;
#pragma unroll
                for (int sl = 0; sl < 2; ++sl)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        tv[sl][0][r] = tb[tfA[r] + (unsigned)(sl * F)]; tv[sl][1][r] = tb[tfA[r] + (unsigned)(sl * F + 16)];
                        tv[sl][2][r] = tb[tfB[r] + (unsigned)(sl * F)]; tv[sl][3][r] = tb[tfB[r] + (unsigned)(sl * F + 16)];
                    }
                if constexpr (!LAST) {
                    tv[2][0] = r16::load_block(p.phi0_tab + trA + (unsigned)(2 * F), 2 * nbo, q); tv[2][1] = r16::load_block(p.phi0_tab + trA + (unsigned)(2 * F), 2 * nbo + 1, q);
                    tv[2][2] = r16::load_block(p.phi0_tab + trB + (unsigned)(2 * F), 2 * nbo, q); tv[2][3] = r16::load_block(p.phi0_tab + trB + (unsigned)(2 * F), 2 * nbo + 1, q);
                }
            }
            {   // ds: invariant message, summed over incoming edges
                f32x4 a0, a1, b0, b1;
                out3(2, nbo, a0, a1, b0, b1);
                if constexpr (GENERAL) put_rows(a0, a1, b0, b1, fo);
                else {
                    emitA(a0, a1, fo);
                    emitB(b0, b1, fo);
                }
            }
            TI_STAMP();
            if constexpr (!LAST) {
                // de: edge state update e += de of both directions in the ROW layout (lane (j, q): row j, features 16 (2 nbo) + 4q .. and
                // 16 (2 nbo + 1) + 4q ..): the same two chunks with the operands the other way round; the old row is loaded before the
                // products and stored after them -- one owner per row, no atomics
                f32x4 a0 = r16::load_block(vec + (EV::P_B2 + 3) * F, 2 * nbo, q), a1 = r16::load_block(vec + (EV::P_B2 + 3) * F, 2 * nbo + 1, q);
                f32x4 b0 = a0, b1 = a1;
                f32x4 w0 = r16::load_block(vec + (EV::W_B2 + 3) * F, 2 * nbo, q), w1 = r16::load_block(vec + (EV::W_B2 + 3) * F, 2 * nbo + 1, q);
                float* const ea = p.e + erowA * F + (TAILS ? erow_l : (unsigned)(j * F));
                float* const eb = p.e + erowB * F + (TAILS ? erow_l : (unsigned)(j * F));
                f32x4 oA0, oA1, oB0, oB1;
                if (FIRST) {
                    const float* em = p.edge_emb + prow_type(meta) * F;
                    oA0 = r16::load_block(em, 2 * nbo, q); oA1 = r16::load_block(em, 2 * nbo + 1, q);
                    oB0 = oA0; oB1 = oA1;
                } else {
                    oA0 = oA1 = oB0 = oB1 = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (row_ok) {
                        oA0 = r16::load_block(ea, 2 * nbo, q); oA1 = r16::load_block(ea, 2 * nbo + 1, q);
                        oB0 = r16::load_block(eb, 2 * nbo, q); oB1 = r16::load_block(eb, 2 * nbo + 1, q);
                    }
                }
                if constexpr (TABLE) {
                    a0 = tv[2][0]; a1 = tv[2][1]; b0 = tv[2][2]; b1 = tv[2][3];
                } else {
                    r16::gemm_x2_on_pipe<false>(a0, a1, b0, b1, h2A, h2B, pipe, lane);
                    pipe.release();
                }
                r16::gemm_on_pipe<false>(w0, w1, g2, pipe, lane);
                pipe.release();
                w0 *= wrow; w1 *= wrow;
                if ((TAILS ? okR : group_ok) && row_ok) {
                    r16::store_block(ea, 2 * nbo, q, oA0 + a0 * w0); r16::store_block(ea, 2 * nbo + 1, q, oA1 + a1 * w1);
                    r16::store_block(eb, 2 * nbo, q, oB0 + b0 * w0); r16::store_block(eb, 2 * nbo + 1, q, oB1 + b1 * w1);
                }
            }
            TI_STAMP();
            if constexpr (GENERAL) {
                // equivariant message, row by row: sed * dir + gates * v[src] + cg * dir x v[dst] (layer 0: the first term alone) of both
                // directions to dvacc of the row's two atoms.  The gate and scale products wait in LDS while the cross-gate products
                // run, like the dv sums of the tile build.
                f32x4 sA0, sA1, sB0, sB1, gA0 = {0, 0, 0, 0}, gA1 = {0, 0, 0, 0}, gB0 = {0, 0, 0, 0}, gB1 = {0, 0, 0, 0};
                f32x4 cA0 = {0, 0, 0, 0}, cA1 = {0, 0, 0, 0}, cB0 = {0, 0, 0, 0}, cB1 = {0, 0, 0, 0};
                out3(1, nbo, sA0, sA1, sB0, sB1);
                if (!FIRST) out3(0, nbo, gA0, gA1, gB0, gB1);
                if constexpr (FOLD) {
                    zpark[0] = sA0; zpark[64] = sA1; zpark[128] = sB0; zpark[192] = sB1;
                    zpark[256] = gA0; zpark[320] = gA1; zpark[384] = gB0; zpark[448] = gB1;
                    out3(4, nbo, cA0, cA1, cB0, cB1);
                    sA0 = zpark[0]; sA1 = zpark[64]; sB0 = zpark[128]; sB1 = zpark[192];
                    gA0 = zpark[256]; gA1 = zpark[320]; gB0 = zpark[384]; gB1 = zpark[448];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const f32x4 dir = *reinterpret_cast<const f32x4*>(scratch + (4 * q + r) * 4);     // direction A's; B's is its negative
                    float vI[3][2] = {}, vJ[3][2] = {};
                    if (!FIRST) {
                        const float* vp = v_g + (gI[r] * (unsigned)(3 * F) + (unsigned)fo);
                        const float* vq = v_g + (gJ[r] * (unsigned)(3 * F) + (unsigned)fo);
#pragma unroll
                        for (int c = 0; c < 3; ++c) { vI[c][0] = vp[c * F]; vI[c][1] = vp[c * F + 16]; vJ[c][0] = vq[c * F]; vJ[c][1] = vq[c * F + 16]; }
                    }
                    float zA[3][2], zB[3][2];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        zA[c][0] = sA0[r] * dir[c]; zA[c][1] = sA1[r] * dir[c];
                        zB[c][0] = -(sB0[r] * dir[c]); zB[c][1] = -(sB1[r] * dir[c]);
                        if (!FIRST) {
                            zA[c][0] = fmaf(gA0[r], vI[c][0], zA[c][0]); zA[c][1] = fmaf(gA1[r], vI[c][1], zA[c][1]);
                            zB[c][0] = fmaf(gB0[r], vJ[c][0], zB[c][0]); zB[c][1] = fmaf(gB1[r], vJ[c][1], zB[c][1]);
                        }
                    }
                    if constexpr (FOLD) {
                        float kA[3][2], kB[3][2];
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            kA[c][0] = cA0[r] * dir[c]; kA[c][1] = cA1[r] * dir[c];
                            kB[c][0] = -(cB0[r] * dir[c]); kB[c][1] = -(cB1[r] * dir[c]);
                        }
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
#pragma unroll
                            for (int h = 0; h < 2; ++h) {     // torch.cross(edge_dir, v[dst]): dst J for direction A, I for direction B
                                zA[c][h] += kA[c1][h] * vJ[c2][h] - kA[c2][h] * vJ[c1][h];
                                zB[c][h] += kB[c1][h] * vI[c2][h] - kB[c2][h] * vI[c1][h];
                            }
                        }
                    }
                    if (gok[r])
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            float* dA = acc_ptr(gJ[r], (1 + c) * F + fo);
                            float* dB = acc_ptr(gI[r], (1 + c) * F + fo);
                            row_out(dA, zA[c][0]); row_out(dA + 16, zA[c][1]);
                            row_out(dB, zB[c][0]); row_out(dB + 16, zB[c][1]);
                        }
                }
            } else {   // equivariant message: sum_e (sed * dir_e + gates * v[src_e]) -> dvacc ; sum_e cg * dir_e -> cacc, or folded into dvacc
                f32x4 sA0, sA1, sB0, sB1, gA0 = {0, 0, 0, 0}, gA1 = {0, 0, 0, 0}, gB0 = {0, 0, 0, 0}, gB1 = {0, 0, 0, 0};
                out3(1, nbo, sA0, sA1, sB0, sB1);
                float vI[3][2], vJ[3][2];                // v of I[q] (source of direction A for the lane's four rows) and of J[q]
                if (!FIRST) {
                    const float* vp = v_g + (lIq * (unsigned)(3 * F) + (unsigned)fo);
                    const float* vq = v_g + (lJq * (unsigned)(3 * F) + (unsigned)fo);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        vI[c][0] = vp[c * F]; vI[c][1] = vp[c * F + 16];
                        if (GATHER_EARLY) { vJ[c][0] = vq[c * F]; vJ[c][1] = vq[c * F + 16]; }
                    }
                    out3(0, nbo, gA0, gA1, gB0, gB1);
                }
                f32x4 dir[4];                            // edge_dir of direction A; direction B's is its negative
#pragma unroll
                for (int r = 0; r < 4; ++r) dir[r] = *reinterpret_cast<const f32x4*>(scratch + (4 * q + r) * 4);
                float zA[3][2], zB[3][2];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    f32x4 v0, v1;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        v0[r] = sA0[r] * dir[r][c]; v1[r] = sA1[r] * dir[r][c];
                        if (!FIRST) { v0[r] = fmaf(gA0[r], vI[c][0], v0[r]); v1[r] = fmaf(gA1[r], vI[c][1], v1[r]); }
                    }
                    zA[c][0] = sumA(v0); zA[c][1] = sumA(v1);
                    if (!GATHER_EARLY) putA(zA[c][0], zA[c][1], (1 + c) * F + fo);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    f32x4 v0, v1;
                    float j0[4], j1[4];                  // v[src] of direction B: the J atom of each row
                    if (!FIRST) {
                        if (GATHER_EARLY) { rows4(vJ[c][0], j0); rows4(vJ[c][1], j1); }
                        else
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float* vr = v_g + (lnode_of(prow_molJ(mi[r]), prow_atomJ(mi[r])) * (unsigned)(3 * F) + (unsigned)(c * F + fo));
                                j0[r] = vr[0]; j1[r] = vr[16];
                            }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        v0[r] = -(sB0[r] * dir[r][c]); v1[r] = -(sB1[r] * dir[r][c]);
                        if (!FIRST) { v0[r] = fmaf(gB0[r], j0[r], v0[r]); v1[r] = fmaf(gB1[r], j1[r], v1[r]); }
                    }
                    zB[c][0] = sumB(v0); zB[c][1] = sumB(v1);
                    if (!GATHER_EARLY) putB(zB[c][0], zB[c][1], (1 + c) * F + fo);
                }
                TI_STAMP();
                if constexpr (FOLD) {
                    // cross term folded: every row a lane sums for one slot has the same destination, so the slot's block sum of
                    // cg * dir is crossed with v[dst] here -- sum_rows cg (dir x v[dst]) = (sum_rows cg dir) x v[dst] -- and added to
                    // the dv sums before their atomics.  v[dst]: J[q] for direction A (vJ, lane row q holds J slot q after sumA), I[q]
                    // for direction B (vI).  12 FMAs per lane instead of 12 accumulator atomics and the update kernel's cacc read.
                    // The 12 dv sums wait in LDS while the products run (held in registers, they made the middle and the last layer
                    // spill 45 registers); edge_dir is read from LDS again after them for the same reason.
                    zpark[0] = f32x4{zA[0][0], zA[0][1], zA[1][0], zA[1][1]};
                    zpark[64] = f32x4{zA[2][0], zA[2][1], zB[0][0], zB[0][1]};
                    zpark[128] = f32x4{zB[1][0], zB[1][1], zB[2][0], zB[2][1]};
                    f32x4 cA0, cA1, cB0, cB1;
                    out3(4, nbo, cA0, cA1, cB0, cB1);
                    f32x4 dc[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) dc[r] = *reinterpret_cast<const f32x4*>(scratch + (4 * q + r) * 4);
                    {
                        const f32x4 z0 = zpark[0], z1 = zpark[64], z2 = zpark[128];
                        zA[0][0] = z0[0]; zA[0][1] = z0[1]; zA[1][0] = z0[2]; zA[1][1] = z0[3];
                        zA[2][0] = z1[0]; zA[2][1] = z1[1]; zB[0][0] = z1[2]; zB[0][1] = z1[3];
                        zB[1][0] = z2[0]; zB[1][1] = z2[1]; zB[2][0] = z2[2]; zB[2][1] = z2[3];
                    }
                    float kA[3][2], kB[3][2];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        f32x4 a0, a1, b0, b1;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            a0[r] = cA0[r] * dc[r][c]; a1[r] = cA1[r] * dc[r][c];
                            b0[r] = -(cB0[r] * dc[r][c]); b1[r] = -(cB1[r] * dc[r][c]);
                        }
                        kA[c][0] = sumA(a0); kA[c][1] = sumA(a1);
                        kB[c][0] = sumB(b0); kB[c][1] = sumB(b1);
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {     // torch.cross(edge_dir, v[dst]) summed over the slot's rows of this block
                            zA[c][h] += kA[c1][h] * vJ[c2][h] - kA[c2][h] * vJ[c1][h];
                            zB[c][h] += kB[c1][h] * vI[c2][h] - kB[c2][h] * vI[c1][h];
                        }
                    }
                }
                if (GATHER_EARLY)
#pragma unroll
                    for (int c = 0; c < 3; ++c) { putA(zA[c][0], zA[c][1], (1 + c) * F + fo); putB(zB[c][0], zB[c][1], (1 + c) * F + fo); }
                if (!FIRST && !FOLD) {
                    f32x4 cA0, cA1, cB0, cB1;
                    out3(4, nbo, cA0, cA1, cB0, cB1);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        f32x4 v0, v1;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { v0[r] = cA0[r] * dir[r][c]; v1[r] = cA1[r] * dir[r][c]; }
                        emitA(v0, v1, (4 + c) * F + fo);
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        f32x4 v0, v1;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { v0[r] = -(cB0[r] * dir[r][c]); v1[r] = -(cB1[r] * dir[r][c]); }
                        emitB(v0, v1, (4 + c) * F + fo);
                    }
                }
            }
        }
        if constexpr (TABLE) { if (p.wpad) pipe.release(); }      // an odd chunk count ends with a pad chunk: whole superchunks per row block
    }
    pipe.drain();
#ifdef TI_STAMPS
    if (p.stamps && lane == 0) {          // whole-loop clock pair of every wave: [4 * WAVES * STAMP_SLOTS + 2 * wave id ...]
        const unsigned long long clk1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
        unsigned long long* c = p.stamps + 2048 + 2 * (size_t)gi_raw;
        c[0] = clk1 - clk0; c[1] = rt1 - rt0;
    }
#endif
}
