// Body of painn_jvp_filter_kernel and its masked twin (painn_jvp_kernels.hip).  TI_FILTER_ROWS_GROUP: which block of p.rows a wave
// reads -- its part of the shared template, or its own (group, part) of the per-molecule row words.
{
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = 256 * NB;
    using A16 = r16::Act<NBK>;
    using OP = r16::Opnd<NBK, SPLIT>;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    float* vec = reinterpret_cast<float*>(lds + 4 * CH4);                           // [EV::COUNT][F]
    for (int i = threadIdx.x; i < EV::COUNT * F / 4; i += T)
        reinterpret_cast<f32x4*>(vec)[i] = reinterpret_cast<const f32x4*>(p.vecs)[i];
    PipeDMA<NB, T, 2> pipe;
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);

    const long long gi_raw = (long long)blockIdx.x * WAVES + wave;
    const bool group_ok = gi_raw < p.n_groups;
    const long long gi = group_ok ? gi_raw : p.n_groups - 1;
    const bool first = p.first != 0, last = p.last != 0;
    const long long mg = gi / p.parts;                                                  // molecule group; gi also counts its parts
    const uint32_t* rows = p.rows + (size_t)(TI_FILTER_ROWS_GROUP) * p.nblk * 16;

    for (int blk = 0; blk < p.nblk; ++blk) {
        const uint32_t meta = rows[blk * 16 + j];
        long long pm = mg * p.G + row_mol(meta);
        pm = pm < p.B ? pm : p.B - 1;
        const long long nsrc = pm * p.A + row_src(meta), ndst = pm * p.A + row_dst(meta);
        const size_t prow0 = ((size_t)gi * p.nblk + blk) * 16;
        const float rx = p.x[nsrc * 3 + 0] - p.x[ndst * 3 + 0];
        const float ry = p.x[nsrc * 3 + 1] - p.x[ndst * 3 + 1];
        const float rz = p.x[nsrc * 3 + 2] - p.x[ndst * 3 + 2];
        const float dist = sqrtf(rx * rx + ry * ry + rz * rz);
        // ---- filter branch, (value, d/d|r|) pair
        OP g2, tg2;
        float tg2sc;
        {
            A16 t1, u1;
            {
                OP enc, tenc;
                float tsc;
                {
                    A16 t, u;
                    r16::posenc_dual(t, u, dist / p.length_scale, 1.0f / p.length_scale, q);      // seed d|r| = 1
                    enc.set(t); tsc = tenc.set_tangent(u);
                }
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const f32x4* wl = pipe.acquire();
                    f32x4 a0 = r16::load_block(vec + EV::W_B0 * F, 2 * c, q), a1 = r16::load_block(vec + EV::W_B0 * F, 2 * c + 1, q);
                    f32x4 b0 = Z4, b1 = Z4;
                    r16::gemm_bt2_sc(a0, a1, b0, b1, enc, 1.0f, tenc, tsc, wl, lane);
                    t1.b[2 * c] = a0; t1.b[2 * c + 1] = a1; u1.b[2 * c] = b0; u1.b[2 * c + 1] = b1;
                    pipe.release();
                }
            }
            r16::ln_silu_dual(t1, u1, vec + EV::W_G0 * F, vec + EV::W_BE0 * F, q);
            {
                OP g1, tg1;
                g1.set(t1);
                const float tsc = tg1.set_tangent(u1);
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const f32x4* wl = pipe.acquire();
                    f32x4 a0 = r16::load_block(vec + EV::W_B1 * F, 2 * c, q), a1 = r16::load_block(vec + EV::W_B1 * F, 2 * c + 1, q);
                    f32x4 b0 = Z4, b1 = Z4;
                    r16::gemm_bt2_sc(a0, a1, b0, b1, g1, 1.0f, tg1, tsc, wl, lane);
                    t1.b[2 * c] = a0; t1.b[2 * c + 1] = a1; u1.b[2 * c] = b0; u1.b[2 * c + 1] = b1;
                    pipe.release();
                }
            }
            r16::ln_silu_dual(t1, u1, vec + EV::W_G1 * F, vec + EV::W_BE1 * F, q);
            g2.set(t1); tg2sc = tg2.set_tangent(u1);
        }
        // ---- phi branch forward, LayerNorm statistics parked for the tangent passes
        OP h2;
        {
            f32x4* stp = reinterpret_cast<f32x4*>(p.st) + ((size_t)(gi * p.nblk + blk) * 4 * NBK) * 64 + lane;
            auto park = [&](int which, const A16& v) {
                if (group_ok) {
#pragma unroll
                    for (int nb = 0; nb < NBK; ++nb) stp[(size_t)(which * NBK + nb) * 64] = v.b[nb];
                }
            };
            A16 t1;
            {
                OP ein;
                if (first) r16::load_set(t1, p.edge_emb + row_type(meta) * F, q);
                else       r16::load_set(t1, p.e + (prow0 + j) * F, q);
                const float esc = ein.set_scaled(t1);                          // e: an un-normalised stream
                const float* prow = p.P + (size_t)nsrc * F;
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const f32x4* wl = pipe.acquire();
                    f32x4 a0 = r16::load_block(prow, 2 * c, q), a1 = r16::load_block(prow, 2 * c + 1, q);
                    r16::gemm_bt_sc(a0, a1, ein, esc, wl, lane);
                    t1.b[2 * c] = a0; t1.b[2 * c + 1] = a1;
                    pipe.release();
                }
            }
            {
                A16 nn, kk;
                r16::ln_silu_stats(t1, nn, kk, vec + EV::P_G0 * F, vec + EV::P_BE0 * F, q);
                park(0, nn); park(1, kk);
            }
            {
                OP h1;
                h1.set(t1);
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const f32x4* wl = pipe.acquire();
                    f32x4 a0 = r16::load_block(vec + EV::P_B1 * F, 2 * c, q), a1 = r16::load_block(vec + EV::P_B1 * F, 2 * c + 1, q);
                    r16::gemm_bt(a0, a1, h1, wl, lane);
                    t1.b[2 * c] = a0; t1.b[2 * c + 1] = a1;
                    pipe.release();
                }
            }
            {
                A16 nn, kk;
                r16::ln_silu_stats(t1, nn, kk, vec + EV::P_G1 * F, vec + EV::P_BE1 * F, q);
                park(2, nn); park(3, kk);
            }
            h2.set(t1);
        }
        f32x4* wq = reinterpret_cast<f32x4*>(p.wq) + ((size_t)(gi * p.nblk + blk) * 5 * NB) * 6 * 64 + lane;
        auto put = [&](int c, int nbo) {
            f32x4 a0 = Z4, a1 = Z4, b0 = Z4, b1 = Z4, tb0 = Z4, tb1 = Z4;
            const f32x4* wl0 = pipe.acquire();
            r16::gemm_fl(a0, a1, h2, wl0, lane);
            pipe.release();
            const f32x4* wl1 = pipe.acquire();
            r16::gemm_bt2_sc<NBK, SPLIT, true>(b0, b1, tb0, tb1, g2, 1.0f, tg2, tg2sc, wl1, lane);
            pipe.release();
            const float* bp = vec + (EV::P_B2 + c) * F + 32 * nbo + j;
            const float* bw = vec + (EV::W_B2 + c) * F + 32 * nbo + j;
            if (group_ok) {
                f32x4* o = wq + (size_t)(c * NB + nbo) * 6 * 64;
                o[0] = a0 + bp[0]; o[64] = a1 + bp[16]; o[128] = b0 + bw[0]; o[192] = b1 + bw[16]; o[256] = tb0; o[320] = tb1;
            }
        };
#pragma unroll 1
        for (int nbo = 0; nbo < NB; ++nbo) {          // consumption order of painn_edge_kernel: ds, de, sed, gates, cross gates
            put(2, nbo);
            if (!last) put(3, nbo);
            put(1, nbo);
            if (!first) { put(0, nbo); put(4, nbo); }
        }
    }
    pipe.drain();
}
