// painn_update_kernel_body.inc -- the body of the update kernel (painn_kernels.hip), included once for painn_update_kernel and once
// for painn_update_cls_kernel (TI_UPDATE_SCLS), so that the builds of before keep their names and their code.
// SCLS (layer 0 after an embed per class, painn_host.hip): the incoming s row of a node is its class's, s_cls[cls[molecule]][atom]; the
// full s is still written.  Rows of one class agree bit for bit (painn_phi0_kernels.hip), so the result is that of the full embed.
// KEEP (TI_UPDATE_KEEP; 0 in the builds of before, whose code it leaves instruction for instruction what it was; 1..3 in their
// *_keep_kernel twins of the split path, painn_update_keep.hip): components c < KEEP of v_eff stay in
// fp32 registers from phase A to phase C instead of being parked in dvacc and read back -- the same fp32 values in the same
// expressions, so the results agree bit for bit with KEEP = 0 -- and components c >= KEEP keep the park (DESIGN.md 4.0k).
{
    constexpr bool SCLS = TI_UPDATE_SCLS;
    constexpr int KEEP = TI_UPDATE_KEEP;
    static_assert(KEEP >= 0 && KEEP <= 3 && (KEEP == 0 || (PREC == 1 && NBK <= 8)), "kept rows: the split path up to F = 128");
    static_assert(!SCLS || (PREC == 1 && !FOLDED), "s per class: layer 0 of the split path");
    constexpr bool H16 = PREC == 2;                 // s, v, P are fp16 in HBM (the accumulators stay fp32), hi-only weight chunks
    constexpr int F = 16 * NBK, NB = (F + 31) / 32, WAVES = 4, T = 64 * WAVES, CH4 = update_chunk4(NB, H16);
    using A16 = r16::Act<NBK>;
    using OP = typename r16::OpSel<NBK, PREC>::type;
    extern __shared__ f32x4 lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
    constexpr int SC = update_superchunk(NB, H16);
    float* vec = reinterpret_cast<float*>(lds + 2 * SC * CH4);                     // [UV::COUNT][F]
    for (int i = threadIdx.x; i < UV::COUNT * F / 4; i += T)
        reinterpret_cast<f32x4*>(vec)[i] = reinterpret_cast<const f32x4*>(p.vecs)[i];
    PipeDMA<NB, T, SC, CH4> pipe;
    pipe.init(reinterpret_cast<const f32x4*>(p.stream), p.nch, lds, wave, lane);

    const long long node = ((long long)blockIdx.x * WAVES + wave) * 16 + j;
    const bool ok = node < p.N;
    const size_t nd = (size_t)(ok ? node : p.N - 1);
    const size_t vo = nd * 3 * F, so_ = nd * F;   // element offsets of this node's v / s rows (fp32 or fp16 storage)
    float* db = p.dvacc + nd * 3 * F;
    float* cb = p.cacc + nd * 3 * F;
    float* ab = p.dsacc + nd * F;                 // sum of the invariant messages of this layer (edge kernel)
    const float* s_in = nullptr;                  // SCLS: the node's incoming s row, its class's
    if constexpr (SCLS) s_in = p.s_cls + ((size_t)p.cls[nd / (size_t)p.A] * (size_t)p.A + nd % (size_t)p.A) * F;

    // ---- phase A: v_eff = v + dvacc + cacc x v (parked in dvacc, or kept in tk), n2 = |V v_eff|^2 over the 3 components
    A16 n2;
    A16 tk[KEEP > 0 ? KEEP : 1];                    // the kept v_eff rows, live until phase C
    {
        OP ve[3];
        float vsc[3];                               // v is an un-normalised stream: per-row scales of the split operands
        {
            A16 t[3];                               // feature block outermost: v, dvacc and cacc are each read ONCE (all three components of a
#pragma unroll                                      // block are needed for the cross product; re-reading them per component missed L2)
            for (int nb = 0; nb < NBK; ++nb) {
                f32x4 vv[3], kk[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    vv[c] = p.first_layer ? f32x4{0, 0, 0, 0} : r16::load_state<H16>(p.v, vo + c * F, nb, q);
                    kk[c] = p.first_layer || FOLDED ? f32x4{0, 0, 0, 0} : r16::load_block(cb + c * F, nb, q);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                    const f32x4 dd = r16::load_block(db + c * F, nb, q);
                    if (FOLDED) t[c].b[nb] = vv[c] + dd;
                    else t[c].b[nb] = (vv[c] + dd) + (kk[c1] * vv[c2] - kk[c2] * vv[c1]);      // torch.cross(edge_dir, v[dst]) summed over edges
                    if (ok && c >= KEEP) r16::store_block(db + c * F, nb, q, t[c].b[nb]);
                    // a kept block has no store that needs it here: pinned, or the compiler sinks the sum to its first use and keeps
                    // its up to seven addends alive in its place -- the rows then spill (profiles/update_keep_resources.txt)
                    if constexpr (KEEP > 0) { if (c < KEEP) asm volatile("" : "+v"(t[c].b[nb])); }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (KEEP == 0) vsc[c] = ve[c].set_scaled(t[c]);
                else if (c >= KEEP) vsc[c] = ve[c].set_scaled(t[c]);
                else tk[c] = t[c];
            }
        }
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) n2.b[nb] = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // a kept row's operand is rebuilt at every chunk visit (set_scaled of the same row gives the same bits): holding the three
                // operands beside the three rows does not fit the register budget of two workgroups per CU
                if constexpr (KEEP > 0) { if (c < KEEP) vsc[c] = ve[c].set_scaled(tk[c]); }
                f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
                r16::gemm_bt(a0, a1, ve[c], wl, lane);                   // vv = V v  (of the scaled rows)
                a0 *= vsc[c]; a1 *= vsc[c];
                n2.b[2 * ch] += a0 * a0; n2.b[2 * ch + 1] += a1 * a1;
            }
            pipe.release();
        }
    }
    // ---- phase B: MLP([ |vv| , s ])
    A16 snew;                                       // s + ds, then s after the update (phase D's operand): read once, kept in registers
    OP h2;
    {
        A16 t;
#pragma unroll
        for (int nb = 0; nb < NBK; ++nb) t.b[nb] = r16::load_block(vec + UV::B0 * F, nb, q);
        {
            OP nn;
            float nsc;
            {
                A16 u;
#pragma unroll
                for (int nb = 0; nb < NBK; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) u.b[nb][r] = sqrtf(n2.b[nb][r]);
                nsc = nn.set_scaled(u);
            }
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                f32x4 g0 = {0, 0, 0, 0}, g1 = {0, 0, 0, 0};
                r16::gemm_bt(g0, g1, nn, wl, lane);
                t.b[2 * ch] += g0 * nsc; t.b[2 * ch + 1] += g1 * nsc;
                pipe.release();
            }
        }
        {
            OP ss;
            float ssc;
#pragma unroll
            for (int nb = 0; nb < NBK; ++nb) {
                if constexpr (SCLS) snew.b[nb] = r16::load_block(s_in, nb, q) + r16::load_block(ab, nb, q);
                else snew.b[nb] = r16::load_state<H16>(p.s, so_, nb, q) + r16::load_block(ab, nb, q);      // s += ds
            }
            ssc = ss.set_scaled(snew);
#pragma unroll
            for (int ch = 0; ch < NB; ++ch) {
                const f32x4* wl = pipe.acquire();
                f32x4 g0 = {0, 0, 0, 0}, g1 = {0, 0, 0, 0};
                r16::gemm_bt(g0, g1, ss, wl, lane);
                t.b[2 * ch] += g0 * ssc; t.b[2 * ch + 1] += g1 * ssc;
                pipe.release();
            }
        }
        r16::ln_silu(t, vec + UV::G0 * F, vec + UV::BE0 * F, q);
        OP h1;
        h1.set(t);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = r16::load_block(vec + UV::B1 * F, 2 * ch, q), a1 = r16::load_block(vec + UV::B1 * F, 2 * ch + 1, q);
            r16::gemm_bt(a0, a1, h1, wl, lane);
            t.b[2 * ch] = a0; t.b[2 * ch + 1] = a1;
            pipe.release();
        }
        r16::ln_silu(t, vec + UV::G1 * F, vec + UV::BE1 * F, q);
        h2.set(t);
    }
    // output chunks: [scale_squared_norm, add_invariant] per 32-feature block, then gates
#pragma unroll
    for (int ch = 0; ch < NB; ++ch) {
        const f32x4* wl = pipe.acquire();
        f32x4 q0 = r16::load_block(vec + (UV::B2 + 1) * F, 2 * ch, q), q1 = r16::load_block(vec + (UV::B2 + 1) * F, 2 * ch + 1, q);
        r16::gemm_bt(q0, q1, h2, wl, lane);
        pipe.release();
        wl = pipe.acquire();
        f32x4 a0 = r16::load_block(vec + (UV::B2 + 2) * F, 2 * ch, q), a1 = r16::load_block(vec + (UV::B2 + 2) * F, 2 * ch + 1, q);
        r16::gemm_bt(a0, a1, h2, wl, lane);
        pipe.release();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int nb = 2 * ch + k;
            f32x4 so = snew.b[nb];
            const f32x4 qq = k ? q1 : q0, aa = k ? a1 : a0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float n = sqrtf(n2.b[nb][r]);
                so[r] = so[r] + ((n * n) * qq[r] + aa[r]);              // s += vv_norm**2 * scale + add
            }
            snew.b[nb] = so;
            if (ok) {
                r16::store_state<H16>(p.s, so_, nb, q, so);
                if (p.zero_acc) r16::store_block(ab, nb, q, f32x4{0, 0, 0, 0});
            }
        }
    }
    A16 gg;
#pragma unroll
    for (int ch = 0; ch < NB; ++ch) {
        const f32x4* wl = pipe.acquire();
        f32x4 a0 = r16::load_block(vec + UV::B2 * F, 2 * ch, q), a1 = r16::load_block(vec + UV::B2 * F, 2 * ch + 1, q);
        r16::gemm_bt(a0, a1, h2, wl, lane);
        gg.b[2 * ch] = a0; gg.b[2 * ch + 1] = a1;
        pipe.release();
    }
    // ---- phase C: v = v_eff + (U v_eff) * gates ; reset the accumulators for the next layer.  One spatial component at a time (the
    // stream holds U three times): the v_eff row (kept, or parked and read once) serves as operand AND as the value the update is added to
    // -- with the three components sharing each chunk visit it had to be read a second time, and that read missed L2.
    if constexpr (KEEP == 0) {
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        A16 t;
        r16::load_set(t, db + c * F, q);
        OP vc;
        const float usc = vc.set_scaled(t);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
            r16::gemm_bt(a0, a1, vc, wl, lane);
            a0 *= usc; a1 *= usc;
            if (ok) {
                r16::store_state<H16>(p.v, vo + c * F, 2 * ch, q, t.b[2 * ch] + a0 * gg.b[2 * ch]);
                r16::store_state<H16>(p.v, vo + c * F, 2 * ch + 1, q, t.b[2 * ch + 1] + a1 * gg.b[2 * ch + 1]);
                if (p.zero_acc) {
                    r16::store_block(db + c * F, 2 * ch, q, f32x4{0, 0, 0, 0});
                    r16::store_block(db + c * F, 2 * ch + 1, q, f32x4{0, 0, 0, 0});
                    if (!FOLDED) {
                        r16::store_block(cb + c * F, 2 * ch, q, f32x4{0, 0, 0, 0});
                        r16::store_block(cb + c * F, 2 * ch + 1, q, f32x4{0, 0, 0, 0});
                    }
                }
            }
            pipe.release();
        }
    }
    } else {
    // the same component step for a kept row (unrolled: registers are not indexed at run time) and for a parked one, read back as above
    const auto component = [&](const int c, const A16& t) {
        OP vc;
        const float usc = vc.set_scaled(t);
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
            r16::gemm_bt(a0, a1, vc, wl, lane);
            a0 *= usc; a1 *= usc;
            if (ok) {
                r16::store_state<H16>(p.v, vo + c * F, 2 * ch, q, t.b[2 * ch] + a0 * gg.b[2 * ch]);
                r16::store_state<H16>(p.v, vo + c * F, 2 * ch + 1, q, t.b[2 * ch + 1] + a1 * gg.b[2 * ch + 1]);
                if (p.zero_acc) {
                    r16::store_block(db + c * F, 2 * ch, q, f32x4{0, 0, 0, 0});
                    r16::store_block(db + c * F, 2 * ch + 1, q, f32x4{0, 0, 0, 0});
                    if (!FOLDED) {
                        r16::store_block(cb + c * F, 2 * ch, q, f32x4{0, 0, 0, 0});
                        r16::store_block(cb + c * F, 2 * ch + 1, q, f32x4{0, 0, 0, 0});
                    }
                }
            }
            pipe.release();
        }
    };
#pragma unroll
    for (int c = 0; c < KEEP; ++c) component(c, tk[c]);
#pragma unroll 1
    for (int c = KEEP; c < 3; ++c) {
        A16 t;
        r16::load_set(t, db + c * F, q);
        component(c, t);
    }
    }
    // ---- phase D: P for the next message block
    if (HAS_NEXT) {
        OP sn;
        float psc;
        {
            psc = sn.set_scaled(snew);               // the rows written above, still in registers
        }
#pragma unroll
        for (int ch = 0; ch < NB; ++ch) {
            const f32x4* wl = pipe.acquire();
            f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
            r16::gemm_bt(a0, a1, sn, wl, lane);
            a0 = r16::load_block(vec + UV::PB0 * F, 2 * ch, q) + a0 * psc; a1 = r16::load_block(vec + UV::PB0 * F, 2 * ch + 1, q) + a1 * psc;
            pipe.release();
            if (ok) { r16::store_state<H16>(p.P, nd * F, 2 * ch, q, a0); r16::store_state<H16>(p.P, nd * F, 2 * ch + 1, q, a1); }
        }
    }
    pipe.drain();
}
