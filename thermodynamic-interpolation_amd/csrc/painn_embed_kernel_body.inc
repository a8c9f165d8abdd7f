// painn_embed_kernel_body.inc -- the body of the embed kernel (painn_kernels.hip), included once for painn_embed16_kernel and once for
// painn_embed16_cls_kernel (TI_EMBED_REP), so that the builds of before keep their names and their code.
// REP (embed per class, painn_host.hip): row n of the launch is (class n / A, atom n % A); it reads the cond rows of the class's
// representative p.rep[class] and writes the compact s_cls / P_cls [n_cls * A][F].
{
    constexpr bool REP = TI_EMBED_REP;
    static_assert(!REP || (PREC == 1 && !TV), "embed per class: the split path at one t");
    constexpr bool H16 = PREC == 2;
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = update_chunk4(NB, H16);
    using A16 = r16::Act<NBK>;
    using OP = typename r16::OpSel<NBK, PREC>::type;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    PipeDMA<NB, T, 2, CH4> pipe;
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);
    const long long node = ((long long)blockIdx.x * WAVES + wave) * 16 + j;
    const bool ok = node < p.N;
    const long long nd = ok ? node : p.N - 1;
    long long cnd = nd;                             // the node whose cond rows this row reads
    if constexpr (REP) cnd = (long long)p.rep[nd / p.A] * p.A + nd % p.A;

    A16 acc;
#pragma unroll
    for (int nb = 0; nb < NBK; ++nb) acc.b[nb] = r16::load_block(p.mlp.b0, nb, q);
#pragma unroll
    for (int seg = 0; seg < NSEG; ++seg) {
        OP op;
        float sc = 1.0f;
        {
            A16 in;
            if (seg == 0) {
                r16::load_set(in, p.atom_emb + (size_t)p.atom_ids[nd % p.A] * F, q);
                sc = op.set_scaled(in);                          // an embedding table: any magnitude
            } else if (seg < NSEG - 1) {
                // TemperatureEncoder.forward: (T - mean(temps)) / (max - min), then PositionalEncoder(max_length=temp_length)
                float u = p.cond[cnd * p.ncond + (seg - 1)] - p.temp_mean;
                u = u / p.temp_range;
                r16::posenc_set(in, u / p.temp_length, q);
                op.set(in);
            } else {
                const float tn = TV ? p.tv[nd / p.A] : p.t;     // batch.t = t * ones_like(atoms), or one t per molecule
                r16::posenc_set(in, tn / p.time_length, q);
                op.set(in);
            }
        }
        const float inv = r16::pow2_inverse(sc);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = acc.b[2 * ch] * inv, a1 = acc.b[2 * ch + 1] * inv;     // exact: sc is a power of two
            r16::gemm_bt(a0, a1, op, wl, lane);
            acc.b[2 * ch] = a0 * sc; acc.b[2 * ch + 1] = a1 * sc;
            pipe.release();
        }
    }
    r16::ln_silu(acc, p.mlp.g0, p.mlp.be0, q);
    A16 t;
    {
        OP h1;
        h1.set(acc);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = r16::load_block(p.mlp.b1, 2 * ch, q), a1 = r16::load_block(p.mlp.b1, 2 * ch + 1, q);
            r16::gemm_bt(a0, a1, h1, wl, lane);
            t.b[2 * ch] = a0; t.b[2 * ch + 1] = a1;
            pipe.release();
        }
    }
    r16::ln_silu(t, p.mlp.g1, p.mlp.be1, q);
    A16 sset;
    {
        OP h2;
        h2.set(t);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = r16::load_block(p.mlp.b2, 2 * ch, q), a1 = r16::load_block(p.mlp.b2, 2 * ch + 1, q);
            r16::gemm_bt(a0, a1, h2, wl, lane);
            sset.b[2 * ch] = a0; sset.b[2 * ch + 1] = a1;
            pipe.release();
        }
    }
    if (ok) {
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) r16::store_state<H16>(p.s, (size_t)node * F, nb, q, sset.b[nb]);
    }
    {
        OP sn;
        const float psc = sn.set_scaled(sset), pinv = r16::pow2_inverse(psc);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = r16::load_block(p.pb0, 2 * ch, q) * pinv, a1 = r16::load_block(p.pb0, 2 * ch + 1, q) * pinv;
            r16::gemm_bt(a0, a1, sn, wl, lane);
            pipe.release();
            if (ok) {
                r16::store_state<H16>(p.P, (size_t)node * F, 2 * ch, q, a0 * psc);
                r16::store_state<H16>(p.P, (size_t)node * F, 2 * ch + 1, q, a1 * psc);
            }
        }
    }
    pipe.drain();
}
