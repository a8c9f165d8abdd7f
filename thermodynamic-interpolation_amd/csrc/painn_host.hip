// painn_host.hip -- host side of a PaiNN evaluation: HBM workspace, the launch sequence of one drift evaluation (with or without
// tangent passes), the divergence / Hutchinson chunk loops on top of it, and the per-molecule graph state.
#include "ti_handle.hpp"

namespace ti {

void ensure_painn_ws(ti_handle* h, long long B)
{
    if (B <= h->cap) return;
    const size_t A = h->d.n_atoms, F = h->d.n_features, N = (size_t)B * A;
    h->x.alloc(N * 3); h->b1.alloc(N * 3); h->b2.alloc(N * 3); h->xt.alloc(N * 3);
    h->cond.alloc(std::max<size_t>(N * h->ncond, 1));
    const size_t se = h->d.precision == TI_PREC_F16 ? 2 : 1;      // state tensors s, P, v, e: fp16 in the storage mode (2 per float slot)
    h->s.alloc((N * F + se - 1) / se); h->P.alloc((N * F + se - 1) / se);
    h->v.alloc((N * 3 * F + se - 1) / se); h->dvacc.alloc(N * 3 * F); h->cacc.alloc(N * 3 * F); h->dsacc.alloc(N * F);
    h->e.alloc((edge_rows_for(h, B) * F + se - 1) / se);
    // parked geometry of a drift evaluation (painn_edge_kernel.hpp): the encoding operand of every edge row (as many bytes as e) and edge_dir
    h->enc.alloc((edge_rows_for(h, B) * F + se - 1) / se); h->geo.alloc(edge_rows_for(h, B) * 4);
    h->divb.alloc(B); h->div2.alloc(B); h->dl.alloc(B); h->dlscaled.alloc(B);
    h->cap = B;
}

// ---- layer-0 phi table: the class pass of an API call.  Whether a drift of the call then takes the table path is
// decided per evaluation (painn_drift_dev): here only what holds for the whole call.  The class count comes back to the host once
// per call -- the device flag for "more classes than the cap" with it -- so every evaluation's launches are chosen on the host.
void phi0_begin_call(ti_handle* h, const float* cond_dev, long long B, bool eligible)
{
    h->phi0_ncls = 0; h->phi0_found = 0; h->phi0_B = 0; h->phi0_cond = nullptr;
    if (!eligible || !h->phi0_ok || h->active != 2 || h->ragged || h->emask_B > 0 || h->tap >= 0 || h->nblk == 0) return;
    const int A = h->d.n_atoms, F = h->d.n_features;
    grow(h->phi0_cls, (size_t)B); grow(h->phi0_state, (size_t)PHI0_STATE_WORDS);
    grow(h->phi0_tab, (size_t)TI_PHI0_MAX_CLASSES * A * PHI0_TYPES * 3 * F);
    if (h->embed_cls_on) { grow(h->s_cls, (size_t)TI_PHI0_MAX_CLASSES * A * F); grow(h->P_cls, (size_t)TI_PHI0_MAX_CLASSES * A * F); }
    int32_t state[PHI0_STATE_WORDS];
    {
        Timed tm(h, TI_KERNEL_PAINN_EMBED);
        HIP_CHECK(hipMemsetAsync(h->phi0_state.p, 0xff, sizeof(state), h->stream));
        Phi0ClassParams p{};
        p.cond = reinterpret_cast<const uint32_t*>(cond_dev); p.words = A * h->ncond; p.B = B; p.state = h->phi0_state.p; p.cls = h->phi0_cls.p;
        HIP_CHECK(launch_phi0_classes(p, h->stream));
    }
    HIP_CHECK(hipMemcpyAsync(state, h->phi0_state.p, sizeof(state), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    int n = 0;
    while (n < TI_PHI0_MAX_CLASSES && state[n] >= 0) ++n;
    const bool over = state[TI_PHI0_MAX_CLASSES] == 1;
    h->phi0_found = over ? TI_PHI0_MAX_CLASSES + 1 : n;
    if (over) return;
    h->phi0_ncls = n; h->phi0_B = B; h->phi0_cond = cond_dev;
}
void phi0_end_call(ti_handle* h) { h->phi0_ncls = 0; h->phi0_B = 0; h->phi0_cond = nullptr; }

// ---- forward-mode derivative: tangent workspace over ceil(B/G)*D*G virtual molecules (painn_jvp_kernels.hip header)
long long jvp_virtual_molecules(const ti_handle* h, long long B, int D) { return (B + h->G - 1) / h->G * D * h->G; }

size_t jvp_bytes_per_vm(const ti_handle* h)
{
    const size_t A = h->d.n_atoms, F = h->d.n_features;
    const size_t erows = ((size_t)h->parts * h->nblk * ti::EDGE_ROWS_PER_BLOCK + h->G - 1) / h->G;
    return (A * F * 12 + erows * F + A * 3) * sizeof(float);
}

void ensure_jvp_ws(ti_handle* h, long long B, int D)
{
    const long long VB = jvp_virtual_molecules(h, B, D);
    const size_t A = h->d.n_atoms, F = h->d.n_features, N = (size_t)VB * A;
    const size_t pgroups = ((size_t)B + h->G - 1) / h->G * h->parts;
    const size_t wq_floats = std::max<size_t>(pgroups * h->nblk * 5 * h->NB * 6 * 64 * 4, 4);
    const size_t st_floats = std::max<size_t>(pgroups * h->nblk * 4 * (2 * h->NB) * 64 * 4, 4);
    grow(h->wq, wq_floats);
    grow(h->phist, st_floats);
    const size_t ns_floats = (((size_t)B * A + 15) / 16) * 13 * (2 * h->NB) * 64 * 4;
    grow(h->nodest, ns_floats);
    const size_t te_floats = (size_t)VB / h->G * h->parts * h->nblk * ti::EDGE_ROWS_PER_BLOCK * F;
    grow(h->te, te_floats);
    if (VB <= h->jvp_cap) return;
    if (N >= ((size_t)1 << 31)) throw std::invalid_argument("too many tangent nodes in one pass (lower TI_JVP_WS_GB)");
    h->ts.alloc(N * F); h->tP.alloc(N * F); h->tdsacc.alloc(N * F);
    h->tv.alloc(N * 3 * F); h->tdvacc.alloc(N * 3 * F); h->tcacc.alloc(N * 3 * F);
    h->tout.alloc(N * 3);
    h->jvp_cap = VB;
}

// molecules per tangent pass with D directions each, from the HBM budget TI_JVP_WS_GB (default 48 GB of tangent state)
long long jvp_chunk_molecules(const ti_handle* h, int D)
{
    double gb = 48.0;
    if (const char* e = std::getenv("TI_JVP_WS_GB")) gb = std::max(0.001, std::atof(e));
    const double per_mol = (double)jvp_bytes_per_vm(h) * D;
    const long long by_mem = (long long)(gb * 1e9 / per_mol);
    const long long by_index = (long long)(((size_t)1 << 31) - 1) / ((long long)D * h->d.n_atoms) - h->G;
    const long long c = std::max<long long>(1, std::min(by_mem, by_index));
    return c >= h->G ? c / h->G * h->G : c;                  // whole primal groups per pass
}

#ifdef TI_STAMPS      // diagnostic build only (tools/gpu_clock.sh): shader-clock stamps of one message-kernel launch, printed to stderr
static DevBuf<unsigned long long> stamp_buf;
static size_t stamps_len(long long groups) { return 2048 + 2 * (size_t)groups + 16; }

// the cleared stamp buffer for a launch over `groups` waves; NULL unless TI_STAMPS_DUMP is set
static unsigned long long* stamps_arm(long long groups, hipStream_t st)
{
    if (!std::getenv("TI_STAMPS_DUMP")) return nullptr;
    const size_t n_st = stamps_len(groups);
    grow(stamp_buf, n_st);
    HIP_CHECK(hipMemsetAsync(stamp_buf.p, 0, n_st * 8, st));
    return stamp_buf.p;
}

static void stamps_dump(const ti_handle* h, const unsigned long long* stamps, long long groups, hipStream_t st)
{
    if (!stamps) return;
    const size_t n_st = stamps_len(groups);
    std::vector<unsigned long long> hs(n_st);
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipMemcpy(hs.data(), stamps, n_st * 8, hipMemcpyDeviceToHost));
    for (int w = 0; w < 32; ++w) {
        if (!hs[(size_t)w * 64 + 1]) continue;
        std::fprintf(stderr, "STAMP %d:", w);
        for (int k = 1; k < 64 && hs[(size_t)w * 64 + k]; ++k) std::fprintf(stderr, " %llu", hs[(size_t)w * 64 + k] - hs[(size_t)w * 64 + k - 1]);
        std::fprintf(stderr, "\n");
    }
    std::vector<double> clk;
    for (long long g2 = 0; g2 < groups; ++g2) { const auto c = hs[2048 + 2 * g2], r = hs[2048 + 2 * g2 + 1]; if (r) clk.push_back(100e6 * (double)c / (double)r); }
    std::sort(clk.begin(), clk.end());
    if (!clk.empty()) std::fprintf(stderr, "INKERNEL_CLOCK_GHZ median %.4f  p10 %.4f  p90 %.4f  waves %zu  layout %d  precision %d\n", clk[clk.size() / 2] / 1e9,
                                   clk[clk.size() / 10] / 1e9, clk[clk.size() * 9 / 10] / 1e9, clk.size(), h->active, h->d.precision);
}
#endif

// one drift evaluation, everything on h->stream; x_dev / out_dev are device pointers [B*A*3].  With `jr` the tangent
// kernels run in lock step: each reads the primal state its layer's primal kernel is about to overwrite.
// tv (device, [B], may be NULL): one time per molecule instead of t (the embed kernel's per-molecule instantiation).
// b0: the call's first molecule of this batch (the divergence passes run the call in chunks): the edge mask rows it starts at.
void painn_drift_dev(ti_handle* h, const float* x_dev, float t, const float* cond_dev, long long B, float* out_dev,
                     const JvpRun* jr, const float* tv, long long b0)
{
    const int A = h->d.n_atoms, F = h->d.n_features, L = h->d.n_layers, NB = h->NB;
    const long long N = B * A, groups = (B + h->G - 1) / h->G * h->parts;         // edge-kernel waves: (molecule group, part)
    hipStream_t st = h->stream;
    const bool split = h->d.precision == TI_PREC_F16X2;
    const int prec = h->d.precision;
    const uint32_t* mrows = nullptr;          // edge mask in force: the masked twins of the message kernels, on per-group row words
    if (h->emask_B > 0) {
        if (b0 % h->G) throw std::invalid_argument("an edge mask needs whole molecule groups per tangent pass (raise TI_JVP_WS_GB)");
        mrows = masked_rows(h, h->active) + (size_t)(b0 / h->G) * h->parts * h->nblk * ti::EDGE_ROWS_PER_BLOCK;
    }
    if (jr && prec == TI_PREC_F16) throw std::invalid_argument(MSG_NO_FP16_TANGENT);
    if (jr && h->active == 2) throw std::logic_error("tangent passes walk directed edge rows (select_template(.., allow_pair = false))");
    // mixed species: the kernels below never see what the caller left in pad atoms.  They read copies in which every pad atom is
    // parked beside its molecule's atom 0 (distinct, finite places: an off row's 0 * value stays 0) with cond 0 and direction 0.
    const int32_t* nat = h->ragged ? h->natoms_dev.p + b0 : nullptr;
    const float* xdot = jr ? jr->xdot : nullptr;
    if (nat) {
        const size_t n3 = (size_t)B * A * 3, nc = (size_t)B * A * h->ncond;
        grow(h->xpark, n3);
        HIP_CHECK(launch_park_pads(h->xpark.p, x_dev, nat, B, 1, A, 3, 1, st));
        x_dev = h->xpark.p;
        if (nc) {
            grow(h->cpark, nc);
            HIP_CHECK(launch_park_pads(h->cpark.p, cond_dev, nat, B, 1, A, h->ncond, 0, st));
            cond_dev = h->cpark.p;
        }
        if (xdot) {
            grow(h->dpark, n3 * jr->D);
            HIP_CHECK(launch_park_pads(h->dpark.p, xdot, nat, B * jr->D, jr->D, A, 3, 0, st));
            xdot = h->dpark.p;
        }
    }
    const long long VB = jr ? jvp_virtual_molecules(h, B, jr->D) : 0, VN = VB * A, vgroups = VB / h->G * h->parts;
    if (jr) {
        ensure_jvp_ws(h, B, jr->D);
        h->last_VB = B * jr->D; h->last_D = jr->D;
        const size_t nb = (size_t)VN * F * sizeof(float);
        HIP_CHECK(hipMemsetAsync(h->ts.p, 0, nb, st)); HIP_CHECK(hipMemsetAsync(h->tP.p, 0, nb, st));
        HIP_CHECK(hipMemsetAsync(h->tdsacc.p, 0, nb, st));
        HIP_CHECK(hipMemsetAsync(h->tv.p, 0, 3 * nb, st)); HIP_CHECK(hipMemsetAsync(h->tdvacc.p, 0, 3 * nb, st));
        HIP_CHECK(hipMemsetAsync(h->tcacc.p, 0, 3 * nb, st));
    }
    const size_t vbytes = (size_t)N * 3 * F * sizeof(float);
    // With first-touch accumulators (every atom has incoming edges) nothing needs zeroing: layer 0's edge kernel replaces dsacc and
    // dvacc, its update kernel does not read v and cacc (zero by definition), every later layer replaces all three.  The forward-mode
    // passes read the primal v and cacc of layer 0 themselves, and with no layers the readout reads v: then they are cleared.
    const bool ft = h->first_touch && h->tap < 0;      // (the debug taps read "state + pending accumulators": they want them zeroed after use)
    if (!ft || jr || L == 0) {
        HIP_CHECK(hipMemsetAsync(h->v.p, 0, prec == TI_PREC_F16 ? vbytes / 2 : vbytes, st));
        HIP_CHECK(hipMemsetAsync(h->cacc.p, 0, vbytes, st));
    }
    if (!ft) {
        HIP_CHECK(hipMemsetAsync(h->dvacc.p, 0, vbytes, st));
        HIP_CHECK(hipMemsetAsync(h->dsacc.p, 0, (size_t)N * F * sizeof(float), st));
    }
    // layer 0 on the phi table: the call's class pass stands for exactly these molecules, t is one for all of them, and nothing that
    // the table builds do not take is in force (a mask or mixed species, a tap, a tangent pass, a directed layout)
    const bool table = h->phi0_ncls > 0 && h->phi0_B == B && h->phi0_cond == cond_dev && b0 == 0 && h->active == 2 && !tv && !jr && !nat && !mrows &&
                       h->tap < 0 && h->nblk > 0 && L > 0;
    h->phi0_last = table ? 1 : 0;
    // embed per class: on the table path the embedding has two readers, the table kernel (P of the class representatives) and layer 0's
    // update (s, once), and a class's rows agree bit for bit -- the launch covers (class, atom) rows alone, into s_cls / P_cls
    const bool embed_cls = table && h->embed_cls_on;
    h->embed_cls_last = embed_cls ? 1 : 0;
    {
        EmbedParams p{};
        p.stream = h->S(h->st_embed16); p.nch = h->st_embed16.nch; p.mlp = h->vec(h->embed);
        p.pb0 = L > 0 ? h->F(h->phi[0].b0) : h->F(h->embed.b2);
        p.atom_emb = h->F(h->atom_emb); p.atom_ids = h->atom_ids.p; p.cond = cond_dev; p.ncond = h->ncond; p.A = A; p.N = N;
        p.t = t; p.tv = tv; p.temp_length = h->d.temp_length; p.time_length = h->d.time_length; p.temp_mean = h->d.temp_mean; p.temp_range = h->d.temp_range;
        p.s = h->s.p; p.P = h->P.p;
        if (embed_cls) { p.N = (long long)h->phi0_ncls * A; p.rep = h->phi0_state.p; p.s = h->s_cls.p; p.P = h->P_cls.p; }
        Timed tm(h, TI_KERNEL_PAINN_EMBED);
        HIP_CHECK(launch_embed(NB, h->nE, prec, p, st));
    }
    if (table) {
        Phi0TableParams p{};
        p.stream = h->S(h->st_phi0_tab); p.nch = h->st_phi0_tab.nch; p.vecs = h->edge_vecs1.p; p.edge_emb = h->F(h->edge_emb);
        for (int i = 0; i < 6; ++i) p.wscale[i] = h->edge_scale[i];
        p.P = h->P.p; p.state = h->phi0_state.p; p.n_cls = h->phi0_ncls; p.A = A; p.tab = h->phi0_tab.p;
        if (embed_cls) { p.P = h->P_cls.p; p.state = nullptr; }
        Timed tm(h, TI_KERNEL_PAINN_EMBED);
        HIP_CHECK(launch_phi0_table(NB, L == 1, p, st));
    }
    // seeded accumulators: the pair layout on a seeded template, and nothing in force that can take a general row away from its two
    // atoms or that the seeded builds do not take (an edge mask or mixed species; f32 handles have no general blocks at all).  A mask
    // that removes nothing (emask_full) leaves every row word the template's: the message launches are then those of an unmasked batch,
    // so that the two agree bit for bit as they always have (the masked twins add in the first-touch order)
    const bool mask_off = mrows && h->emask_full;
    const bool seeded = h->active == 2 && h->pair_seeded_on && h->n_tile > 0 && h->n_tile < h->nblk && pair_general_build_exists(prec) && (!mrows || mask_off) && !nat && L > 0;
    h->seeded_last = seeded ? 1 : 0;
    const bool tails = seeded && h->pair_tails_on;      // the seeded general launch on super-groups, their last blocks merged
    h->tails_last = tails ? 1 : 0;
    h->update_keep_last = h->update_keep_on && L > 0 ? update_keep_components(NB, prec) : 0;
    h->last_B = B;
    if (h->tap == 0) return;
    for (int l = 0; l < L; ++l) {
        if (jr && h->nblk > 0) {
            {
                JvpFilterParams p{};
                p.stream = h->S(h->st_edge[l]); p.nch = h->st_edge[l].nch; p.vecs = h->edge_vecs.p + (size_t)l * 21 * F;
                p.edge_emb = h->F(h->edge_emb); p.rows = h->rows.p; p.nblk = h->nblk; p.G = h->G; p.parts = h->parts; p.A = A; p.first = l == 0; p.last = l == L - 1;
                p.B = B; p.n_groups = groups; p.length_scale = h->d.length_scale; p.x = x_dev; p.P = h->P.p; p.e = h->e.p;
                p.wq = reinterpret_cast<float4*>(h->wq.p); p.st = reinterpret_cast<float4*>(h->phist.p);
                const bool typed = mrows && !h->ptype.empty();      // per-molecule edge types: the filter pass reads them from the row words
                if (typed) p.rows = mrows;
                Timed tm(h, TI_KERNEL_PAINN_JVP_FILTER);
                HIP_CHECK(launch_jvp_filter(NB, split, p, st, typed));
            }
            JvpEdgeParams p{};
            p.stream = h->S(h->st_jvp_phi[l]); p.nch = h->st_jvp_phi[l].nch; p.pad = h->jvp_phi_pad[l]; p.vecs = h->edge_vecs.p + (size_t)l * 21 * F;
            p.edge_emb = h->F(h->edge_emb); p.rows = h->rows.p; p.slotnode = h->slotnode.p;
            p.nblk = h->nblk; p.G = h->G; p.parts = h->parts; p.A = A; p.D = jr->D; p.first = l == 0; p.last = l == L - 1;
            p.B = B; p.n_groups = vgroups;
            p.x = x_dev; p.xdot = xdot; p.P = h->P.p; p.v = h->v.p; p.e = h->e.p; p.wq = reinterpret_cast<const float4*>(h->wq.p);
            p.st = reinterpret_cast<const float4*>(h->phist.p); p.tP = h->tP.p; p.tv = h->tv.p;
            p.te = h->te.p; p.tdsacc = h->tdsacc.p; p.tdvacc = h->tdvacc.p; p.tcacc = h->tcacc.p;
            if (mrows) p.rows = mrows;
            Timed tm(h, TI_KERNEL_PAINN_JVP_EDGE);
            HIP_CHECK(launch_jvp_edge(NB, split, p, st, mrows != nullptr));
        }
        if (h->nblk > 0) {
            EdgeParams p{};
            p.stream = h->S(h->st_edge[l]); p.nch = h->st_edge[l].nch; p.vecs = h->edge_vecs.p + (size_t)l * 21 * F;
            p.edge_emb = h->F(h->edge_emb); p.rows = h->rows.p; p.slotnode = h->slotnode.p; p.nslots = nullptr;
            p.nblk = h->nblk; p.n_tile = h->n_tile; p.G = h->G; p.parts = h->parts; p.A = A; p.max_slots = h->max_slots; p.B = B; p.n_groups = groups; p.length_scale = h->d.length_scale;
            p.x = x_dev; p.P = h->P.p; p.v = h->v.p; p.dsacc = h->dsacc.p; p.dvacc = h->dvacc.p; p.cacc = h->cacc.p; p.e = h->e.p; p.enc = h->enc.p; p.geo = h->geo.p;
            for (int i = 0; i < 6; ++i) p.wscale[i] = 1.0f;
            if (edge_one_chain(prec)) {     // the message kernel's own stream format (the primal pass of the divergence keeps the other one)
                p.stream = h->S(h->st_edge1[l]); p.nch = h->st_edge1[l].nch; p.vecs = h->edge_vecs1.p + (size_t)l * 21 * F;
                for (int i = 0; i < 6; ++i) p.wscale[i] = h->edge_scale[(size_t)l * 6 + i];
            }
            if (tails) { p.tail_S = h->pair_tail_S; p.tail_r = h->pair_tail_r; }
            if (mrows && !seeded) p.rows = mrows;      // (seeded under a mask that removes nothing: the template's own row words)
            Timed tm(h, TI_KERNEL_PAINN_EDGE);
#ifdef TI_STAMPS
            if (l == 2) p.stamps = stamps_arm(groups, st);
#endif
            const bool on_table = table && l == 0;
            if (on_table) {           // the w chunks alone; phi's three output slices come from the table
                p.stream = h->S(h->st_phi0_w); p.nch = h->st_phi0_w.nch; p.wpad = h->phi0_wpad;
                p.phi0_tab = h->phi0_tab.p; p.cls = h->phi0_cls.p;
            }
            if (h->active == 2) {
                HIP_CHECK(launch_pair(NB, l == 0, l == L - 1, prec, p, st, mrows != nullptr && !seeded, on_table, seeded));
#ifdef TI_STAMPS
                stamps_dump(h, p.stamps, groups, st);
#endif
            } else {
                HIP_CHECK(launch_edge(NB, l == 0, l == L - 1, prec, p, st, mrows != nullptr));
#ifdef TI_STAMPS
                stamps_dump(h, p.stamps, groups, st);
#endif
            }
        }
        if (h->tap == 1 + 2 * l) return;
        if (jr) {
            {
                JvpNodeParams p{};
                p.stream = h->S(h->st_jvp_update[l]); p.nch = h->st_jvp_update[l].nch; p.vecs = h->upd_vecs.p + (size_t)l * 10 * F;
                p.N = N; p.s = h->s.p; p.v = h->v.p; p.dsacc = h->dsacc.p; p.dvacc = h->dvacc.p; p.cacc = h->cacc.p;
                p.ns = reinterpret_cast<float4*>(h->nodest.p);
                Timed tm(h, TI_KERNEL_PAINN_JVP_FILTER);
                HIP_CHECK(launch_jvp_node(NB, split, p, st));
            }
            JvpUpdateParams p{};
            p.stream = h->S(h->st_jvp_update[l]); p.nch = h->st_jvp_update[l].nch; p.vecs = h->upd_vecs.p + (size_t)l * 10 * F;
            p.N = VN; p.B = B; p.A = A; p.D = jr->D; p.G = h->G; p.has_next = l + 1 < L;
            p.v = h->v.p; p.cacc = h->cacc.p; p.ns = reinterpret_cast<const float4*>(h->nodest.p);
            p.ts = h->ts.p; p.tv = h->tv.p; p.tdsacc = h->tdsacc.p; p.tdvacc = h->tdvacc.p; p.tcacc = h->tcacc.p; p.tP = h->tP.p;
            p.zero_acc = !ft;
            Timed tm(h, TI_KERNEL_PAINN_JVP_UPDATE);
            HIP_CHECK(launch_jvp_update(NB, split, p, st));
        }
        {
            UpdateParams p{};
            p.stream = h->S(h->st_update[l]); p.nch = h->st_update[l].nch; p.vecs = h->upd_vecs.p + (size_t)l * 10 * F;
            p.N = N; p.s = h->s.p; p.v = h->v.p; p.dsacc = h->dsacc.p; p.dvacc = h->dvacc.p; p.cacc = h->cacc.p; p.P = h->P.p;
            p.first_layer = l == 0; p.zero_acc = !ft;
            if (embed_cls && l == 0) { p.s_cls = h->s_cls.p; p.cls = h->phi0_cls.p; p.A = A; }      // the full s is first written here
            // after a pair launch that folded the cross term into dvacc, the update kernel that reads neither cacc nor its cross product
            // (cacc is then not written in this layer; the tangent passes, which read it, run on directed launches only)
            const bool folded = h->nblk > 0 && h->active == 2 && l > 0 && pair_folds_cross(prec);
            Timed tm(h, TI_KERNEL_PAINN_UPDATE);
            HIP_CHECK(launch_update(NB, l + 1 < L, prec, p, st, folded, h->update_keep_on));
        }
        if (h->tap == 2 + 2 * l) return;
    }
    if (jr) {
        JvpReadoutParams p{};
        p.stream = h->S(h->st_jvp_readout); p.nch = h->st_jvp_readout.nch; p.vecs = h->jvp_ro_vecs.p; p.b2_gate = h->b2_gate;
        p.N = VN; p.B = B; p.A = A; p.D = jr->D; p.G = h->G; p.s = h->s.p; p.v = h->v.p; p.ts = h->ts.p; p.tv = h->tv.p; p.tout = jr->tout;
        Timed tm(h, TI_KERNEL_PAINN_JVP_READOUT);
        HIP_CHECK(launch_jvp_readout(NB, split, p, st));
    }
    {
        ReadoutParams p{};
        p.stream = h->S(h->st_jvp_readout); p.nch = h->st_jvp_readout.nch; p.mlp = h->vec(h->readout);      // the 16-row image of W0, W1
        p.w2_gate = h->F(h->readout.W2 + F); p.b2_gate = h->b2_gate; p.Vr = h->F(h->Vr);
        p.N = N; p.s = h->s.p; p.v = h->v.p; p.out = out_dev;
        Timed tm(h, TI_KERNEL_PAINN_READOUT);
        HIP_CHECK(launch_readout(NB, prec, p, st));
    }
    if (nat) {            // a pad atom's drift (and the tangent of an explicit direction) is +0 whatever the network made of it
        HIP_CHECK(launch_zero_pads(out_dev, nat, B, 1, A, 3, st));
        if (jr && jr->D == 1) HIP_CHECK(launch_zero_pads(jr->tout, nat, B, 1, A, 3, st));
    }
}

// drift and exact divergence: 3A unit-seed tangent passes per molecule, in chunks that fit the tangent HBM budget
void painn_drift_div_dev(ti_handle* h, const float* x_dev, float t, const float* cond_dev, long long B, float* out_dev, float* div_dev,
                         const float* tv)
{
    const int A = h->d.n_atoms, D = 3 * A;
    const long long chunk = jvp_chunk_molecules(h, D);
    for (long long b0 = 0; b0 < B; b0 += chunk) {
        const long long bc = std::min(chunk, B - b0);
        ensure_jvp_ws(h, bc, D);
        JvpRun jr{D, nullptr, h->tout.p};
        painn_drift_dev(h, x_dev + (size_t)b0 * A * 3, t, cond_dev ? cond_dev + (size_t)b0 * A * h->ncond : nullptr, bc,
                        out_dev + (size_t)b0 * A * 3, &jr, tv ? tv + b0 : nullptr, b0);
        if (h->ragged) HIP_CHECK(launch_div_reduce_ragged(h->tout.p, bc, D, h->G, h->natoms_dev.p + b0, div_dev + b0, h->stream));
        else HIP_CHECK(launch_div_reduce(h->tout.p, bc, D, h->G, div_dev + b0, h->stream));
    }
    h->last_B = std::min(chunk, B);
}

// Hutchinson probes of trajectories traj0 .. traj0 + B - 1 into h->probes [B][k][3A] (include/ti_hip.h ti_painn_drift_div_est),
// drawn once per API call: a rollout integrates with the same probes at every evaluation
void painn_make_probes(ti_handle* h, long long B, int k, uint64_t seed, long long traj0)
{
    const int n3 = 3 * h->d.n_atoms;
    grow(h->probes, (size_t)B * k * n3);
    HIP_CHECK(launch_probes(h->probes.p, seed, traj0, B, k, n3, h->stream));
    if (h->ragged) HIP_CHECK(launch_zero_pads(h->probes.p, h->natoms_dev.p, B * k, k, h->d.n_atoms, 3, h->stream));      // pad components: 0
}

// drift and Hutchinson estimate of the divergence along the k probes of h->probes: D = k explicit tangent directions per molecule,
// in chunks sized for k directions
void painn_drift_div_est_dev(ti_handle* h, const float* x_dev, float t, const float* cond_dev, long long B, int k, float* out_dev,
                             float* est_dev, const float* tv)
{
    const int A = h->d.n_atoms;
    const long long chunk = jvp_chunk_molecules(h, k);
    for (long long b0 = 0; b0 < B; b0 += chunk) {
        const long long bc = std::min(chunk, B - b0);
        ensure_jvp_ws(h, bc, k);
        const float* eps = h->probes.p + (size_t)b0 * k * A * 3;
        JvpRun jr{k, eps, h->tout.p};
        painn_drift_dev(h, x_dev + (size_t)b0 * A * 3, t, cond_dev ? cond_dev + (size_t)b0 * A * h->ncond : nullptr, bc,
                        out_dev + (size_t)b0 * A * 3, &jr, tv ? tv + b0 : nullptr, b0);
        HIP_CHECK(launch_hutch_reduce(h->tout.p, eps, bc, k, A, h->G, est_dev + b0, h->stream));
    }
    h->last_B = std::min(chunk, B);
}

// ------------------------------------------------------------------------------------------------ graph state
// The per-molecule graph state both setters below write: mask m [B][A] (bits of pad atoms cleared here), atom counts (empty: all A),
// edge types (empty: the template's).  Replaces whatever was in force.
int set_graph_state(ti_handle* h, std::vector<uint32_t>& m, std::vector<int32_t>& natoms, std::vector<uint8_t>& ptype, long long B)
{
    const int A = h->d.n_atoms;
    long long n_real = (long long)B * A; bool ragged = false;
    if (!natoms.empty()) {
        n_real = 0;
        for (long long b = 0; b < B; ++b) {
            const int n = natoms[b];
            n_real += n; ragged = ragged || n < A;
            const uint32_t real = n >= 32 ? 0xffffffffu : (1u << n) - 1u;         // sources that are real atoms
            for (int d = 0; d < A; ++d) m[(size_t)b * A + d] = d < n ? m[(size_t)b * A + d] & real : 0u;
        }
    }
    // symmetric over the template: for every template edge s -> d whose reverse is one too, both bits (and, where the edge is present,
    // both types) agree in every molecule
    std::vector<uint32_t> in_tpl(A, 0);          // bit s of in_tpl[d]: s -> d is a template edge
    for (size_t k = 0; k < h->esrc.size(); ++k) in_tpl[h->edst[k]] |= 1u << h->esrc[k];
    bool sym = true;
    for (long long b = 0; b < B && sym; ++b)
        for (int d = 0; d < A && sym; ++d)
            for (int s2 = 0; s2 < A; ++s2) {
                if (!((in_tpl[d] >> s2) & 1u) || !((in_tpl[s2] >> d) & 1u)) continue;
                const uint32_t on = (m[(size_t)b * A + d] >> s2) & 1u;
                if (on != ((m[(size_t)b * A + s2] >> d) & 1u)) { sym = false; break; }
                if (on && !ptype.empty() && ptype[((size_t)b * A + s2) * A + d] != ptype[((size_t)b * A + d) * A + s2]) { sym = false; break; }
            }
    if (h->emask_B == B && m == h->emask && natoms == h->natoms && ptype == h->ptype) return TI_OK;      // the same state again (a mirror class sets it before every call)
    HIP_CHECK(hipStreamSynchronize(h->stream));                   // no launch in flight still reads the row words about to be replaced
    bool full = ptype.empty() && !ragged;                        // nothing removed: every template edge of every molecule is present
    for (long long b = 0; b < B && full; ++b)
        for (int d = 0; d < A && full; ++d) full = (m[(size_t)b * A + d] & in_tpl[d]) == in_tpl[d];
    h->emask.swap(m); h->emask_B = B; h->emask_sym = sym; h->emask_full = full;
    h->natoms.swap(natoms); h->ptype.swap(ptype); h->ragged = ragged; h->n_real = n_real;
    if (ragged) h->natoms_dev.upload(h->natoms); else h->natoms_dev.release();
    for (int t = 0; t < 3; ++t) h->mrows_ok[t] = false;
    return TI_OK;
}

void clear_graph_state(ti_handle* h)
{
    h->emask_B = 0; h->emask_sym = true; h->emask_full = false; h->emask.clear(); h->natoms.clear(); h->ptype.clear(); h->ragged = false; h->n_real = 0;
    for (int t = 0; t < 3; ++t) { h->mrows_ok[t] = false; h->mrows[t].release(); }
}

}  // namespace ti
