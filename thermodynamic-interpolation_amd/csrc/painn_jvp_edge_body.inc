// painn_jvp_edge_body.inc -- the body of the tangent message kernel (painn_jvp_kernels.hip), included once for painn_jvp_edge_kernel
// and once for its masked twin painn_jvp_edge_mask_kernel.  TI_ROWS_GROUP: the index of the wave's row words -- its part of the
// template in the first; its primal (group, part) in the second, whose per-group row words give absent edges the slot 63.
{
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = 256 * NB;
    using A16 = r16::Act<NBK>;
    using OP = r16::Opnd<NBK, SPLIT>;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    float* scratch = reinterpret_cast<float*>(lds + 4 * CH4) + wave * 128;         // [16 rows][8]: edge_dir, d|r|', edge_dir', 0
    float* vec = reinterpret_cast<float*>(lds + 4 * CH4) + WAVES * 128;            // [EV::COUNT][F]
    for (int i = threadIdx.x; i < EV::COUNT * F / 4; i += T)
        reinterpret_cast<f32x4*>(vec)[i] = reinterpret_cast<const f32x4*>(p.vecs)[i];
    PipeDMA<NB, T, 2> pipe;
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);

    // virtual group.  The D directions of a primal group (consecutive virtual groups) read the same primal-pass rows (wq, st: 154 KB per
    // row block at F = 128), the same P / v / e rows; dealt round-robin over the XCDs, every L2 fetched them again from HBM (140 GB
    // read per launch, profiles/r03f_divergence_pmc_summary.txt): neighbours in the logical order share an XCD instead.
    const long long gi_raw = xcd_swizzle(blockIdx.x, gridDim.x) * WAVES + wave;
    const bool group_ok = gi_raw < p.n_groups;
    const long long gi = group_ok ? gi_raw : p.n_groups - 1;
    // gi = (molecule group * D + direction) * P + part
    const long long vmg = gi / p.parts;                                                 // virtual molecule group
    const int part = (int)(gi - vmg * p.parts);
    const long long mg = vmg / p.D;                                                 // molecule group
    const int dsel = (int)(vmg - mg * p.D);                                         // seed direction
    const long long pg = mg * p.parts + part;                                         // primal group (incl. part): rows of e, wq, st
    const uint32_t* rows = p.rows + (size_t)TI_ROWS_GROUP * p.nblk * 16;
    const int32_t* slotnode = p.slotnode + (size_t)part * p.nblk * 16;
    const bool first = p.first != 0, last = p.last != 0;

    for (int blk = 0; blk < p.nblk; ++blk) {
        // ---- geometry of this lane's row and its tangent
        const uint32_t meta = rows[blk * 16 + j];
        long long pm = mg * p.G + row_mol(meta);
        pm = pm < p.B ? pm : p.B - 1;
        const long long nsrc = pm * p.A + row_src(meta), ndst = pm * p.A + row_dst(meta);
        const size_t trow0 = ((size_t)gi * p.nblk + blk) * 16;                       // tangent rows of this block
        {
            const float rx = p.x[nsrc * 3 + 0] - p.x[ndst * 3 + 0];
            const float ry = p.x[nsrc * 3 + 1] - p.x[ndst * 3 + 1];
            const float rz = p.x[nsrc * 3 + 2] - p.x[ndst * 3 + 2];
            float tx, ty, tz;
            if (p.xdot) {                                           // xdot [B][D][A][3]: direction dsel of molecule pm
                const float* xd = p.xdot + (size_t)(pm * p.D + dsel) * p.A * 3;
                const int xs = row_src(meta) * 3, xt = row_dst(meta) * 3;
                tx = xd[xs + 0] - xd[xt + 0];
                ty = xd[xs + 1] - xd[xt + 1];
                tz = xd[xs + 2] - xd[xt + 2];
            } else {                                                // unit seed on (atom, component) = (dsel / 3, dsel % 3)
                const int sa = dsel / 3, sc = dsel - 3 * sa;
                const float sg = (float)((row_src(meta) == sa) - (row_dst(meta) == sa));
                tx = sc == 0 ? sg : 0.f; ty = sc == 1 ? sg : 0.f; tz = sc == 2 ? sg : 0.f;
            }
            const float dist = sqrtf(rx * rx + ry * ry + rz * rz);
            const float ddist = dist > 0.f ? (rx * tx + ry * ty + rz * tz) / dist : 0.f;
            const float den = 1.0f + dist, k = ddist / (den * den);
            if (q == 0) {
                *reinterpret_cast<f32x4*>(scratch + j * 8) = f32x4{rx / den, ry / den, rz / den, ddist};
                *reinterpret_cast<f32x4*>(scratch + j * 8 + 4) = f32x4{tx / den - rx * k, ty / den - ry * k, tz / den - rz * k, 0.f};
            }
        }
        // ---- tangent of phi's hidden layers (first layer: s and e do not depend on x yet, the whole tangent is zero)
        OP th2;
        float th2sc = 1.0f;
        if (!first) {
            const f32x4* stp = reinterpret_cast<const f32x4*>(p.st) + ((size_t)(pg * p.nblk + blk) * 4 * NBK) * 64 + lane;
            auto stat = [&](int which, A16& v) {
#pragma unroll
                for (int nb = 0; nb < NBK; ++nb) v.b[nb] = stp[(size_t)(which * NBK + nb) * 64];
            };
            A16 u1;
            {
                OP tein;
                r16::load_set(u1, p.te + (trow0 + j) * F, q);
                const float tsc = tein.set_tangent(u1);
                const float* tprow = p.tP + (size_t)((vmg * p.G + row_mol(meta)) * p.A + row_src(meta)) * F;
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const f32x4* wl = pipe.acquire();
                    f32x4 b0 = r16::load_block(tprow, 2 * c, q), b1 = r16::load_block(tprow, 2 * c + 1, q);
                    r16::gemm_bt_sc(b0, b1, tein, tsc, wl, lane);
                    u1.b[2 * c] = b0; u1.b[2 * c + 1] = b1;
                    pipe.release();
                }
            }
            {
                A16 nn, kk;
                stat(0, nn); stat(1, kk);
                r16::ln_tangent(u1, nn, kk);
            }
            {
                OP th1;
                const float tsc = th1.set_tangent(u1);
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const f32x4* wl = pipe.acquire();
                    f32x4 b0 = Z4, b1 = Z4;
                    r16::gemm_bt_sc(b0, b1, th1, tsc, wl, lane);
                    u1.b[2 * c] = b0; u1.b[2 * c + 1] = b1;
                    pipe.release();
                }
            }
            {
                A16 nn, kk;
                stat(2, nn); stat(3, kk);
                r16::ln_tangent(u1, nn, kk);
            }
            th2sc = th2.set_tangent(u1);
        } else {
#pragma unroll
            for (int c = 0; c < 2 * NB; ++c) { (void)pipe.acquire(); pipe.release(); }      // keep the stream in phase
        }
        // ---- output layer, flipped (features on lanes, the block's rows 4q + r in registers); see painn_edge_kernel
        uint32_t mi[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) mi[r] = rows[blk * 16 + 4 * q + r];
        // per-atom sums over the block's rows on VALU lane swaps (r16::QuarterSum; a block has at most 4 destination atoms): quarter q
        // of the wave ends up with the 16-row sum of slot q, one atomic instruction per 16-feature half adds every slot of the block
        r16::QuarterSum<4> qs;
#pragma unroll
        for (int r = 0; r < 4; ++r) qs.set_row(r, row_slot(mi[r]));
        int qnode;
        bool qfirst;                                 // first block of that atom: its sums replace the tangent accumulators' contents
        {
            const int sn = slotnode[blk * 16 + q];
            const long long m2 = slot_mol(sn);
            qnode = (sn >= 0 && group_ok && mg * p.G + m2 < p.B) ? (int)((vmg * p.G + m2) * p.A + (sn & 255)) : -1;     // TANGENT node
            qfirst = (sn & SLOT_FIRST_TOUCH) != 0;
        }
        f32x4 dir[4], tdir[4], dd;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dir[r] = *reinterpret_cast<const f32x4*>(scratch + (4 * q + r) * 8);
            tdir[r] = *reinterpret_cast<const f32x4*>(scratch + (4 * q + r) * 8 + 4);
            dd[r] = dir[r][3];
        }
        const f32x4* wq = reinterpret_cast<const f32x4*>(p.wq) + ((size_t)(pg * p.nblk + blk) * 5 * NB) * 6 * 64 + lane;
        // value and tangent of (phi_c + b)(w_c + b) for output chunk c, 32 features as two 16-feature blocks
        auto out_pair = [&](int c, int nbo, f32x4& r0, f32x4& r1, f32x4& d0, f32x4& d1) {
            // raised issue priority from the filter-product loads to the tangent products (mfma_chain.hpp: gemm_on_pipe): +1.5 % on the
            // divergence workload (profiles/r03i_setprio_timing.txt); around the hidden layers' products it changes nothing, and bracketing
            // only the matrix instructions here costs hipcc 680 spilled registers (s_setprio is a scheduling boundary)
            __builtin_amdgcn_s_setprio(1);
            const f32x4* g = wq + (size_t)(c * NB + nbo) * 6 * 64;
            const f32x4 A0 = g[0], A1 = g[64], B0 = g[128], B1 = g[192], Q0 = g[256], Q1 = g[320];
            f32x4 ta0 = Z4, ta1 = Z4;
            const f32x4* wl = pipe.acquire();
            if (!first) r16::gemm_fl_sc(ta0, ta1, th2, th2sc, wl, lane);
            pipe.release();
            r0 = A0 * B0; r1 = A1 * B1;
            d0 = ta0 * B0 + A0 * (dd * Q0); d1 = ta1 * B1 + A1 * (dd * Q1);
            __builtin_amdgcn_s_setprio(0);
        };
        auto emit = [&](const f32x4& v0, const f32x4& v1, float* dst, size_t stride) {
            const float z0 = qs.sum(v0), z1 = qs.sum(v1);
            if (qnode >= 0) { float* d = dst + (size_t)qnode * stride; acc_out(d, z0, qfirst); acc_out(d + 16, z1, qfirst); }
        };

#pragma unroll 1
        for (int nbo = 0; nbo < NB; ++nbo) {
            const int fo = 32 * nbo + j;
            {   // ds
                f32x4 v0, v1, d0, d1;
                out_pair(2, nbo, v0, v1, d0, d1);
                emit(d0, d1, p.tdsacc + fo, F);
            }
            if (!last) {   // de: te += d(de).  Every tangent edge row has ONE owner (this wave), so the update is a plain load / add / store
                // instead of the 32 fire-and-forget atomic instructions per row block it used to be (more than half of this kernel's
                // dword atomics).  Measured: the launch takes the same 46.9 ms either way (profiles/r03f_divergence_*): like the primal
                // message kernel this one is bound by its serial per-wave timeline, not by L2's atomic rate.  The old rows are
                // requested before the products and consumed behind them.
                f32x4 o0 = Z4, o1 = Z4;
                if (!first) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float* ep = p.te + (trow0 + 4 * q + r) * F + fo;
                        o0[r] = ep[0]; o1[r] = ep[16];
                    }
                }
                f32x4 v0, v1, d0, d1;
                out_pair(3, nbo, v0, v1, d0, d1);
                if (group_ok) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* ep = p.te + (trow0 + 4 * q + r) * F + fo;
                        ep[0] = o0[r] + d0[r]; ep[16] = o1[r] + d1[r];
                    }
                }
            }
            {   // equivariant message
                f32x4 sed0, sed1, tsed0, tsed1, gt0 = Z4, gt1 = Z4, tgt0 = Z4, tgt1 = Z4;
                out_pair(1, nbo, sed0, sed1, tsed0, tsed1);
                f32x4 vs[3][2], tvs[3][2];
                if (!first) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        long long pm2 = mg * p.G + row_mol(mi[r]);
                        pm2 = pm2 < p.B ? pm2 : p.B - 1;
                        const float* vp = p.v + (size_t)(pm2 * p.A + row_src(mi[r])) * 3 * F + fo;
                        const float* tp = p.tv + (size_t)((vmg * p.G + row_mol(mi[r])) * p.A + row_src(mi[r])) * 3 * F + fo;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            vs[c][0][r] = vp[c * F]; vs[c][1][r] = vp[c * F + 16];
                            tvs[c][0][r] = tp[c * F]; tvs[c][1][r] = tp[c * F + 16];
                        }
                    }
                    out_pair(0, nbo, gt0, gt1, tgt0, tgt1);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    f32x4 v0, v1;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        v0[r] = tsed0[r] * dir[r][c] + sed0[r] * tdir[r][c];
                        v1[r] = tsed1[r] * dir[r][c] + sed1[r] * tdir[r][c];
                        if (!first) {
                            v0[r] += tgt0[r] * vs[c][0][r] + gt0[r] * tvs[c][0][r];
                            v1[r] += tgt1[r] * vs[c][1][r] + gt1[r] * tvs[c][1][r];
                        }
                    }
                    emit(v0, v1, p.tdvacc + c * F + fo, 3 * F);
                }
                if (!first) {
                    f32x4 cg0, cg1, tcg0, tcg1;
                    out_pair(4, nbo, cg0, cg1, tcg0, tcg1);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        f32x4 v0, v1;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            v0[r] = tcg0[r] * dir[r][c] + cg0[r] * tdir[r][c];
                            v1[r] = tcg1[r] * dir[r][c] + cg1[r] * tdir[r][c];
                        }
                        emit(v0, v1, p.tcacc + c * F + fo, 3 * F);
                    }
                }
            }
        }
        if (p.pad) { (void)pipe.acquire(); pipe.release(); }      // odd chunk count: swallow the pad chunk, stay in phase with the superchunk ring
    }
    pipe.drain();
}
