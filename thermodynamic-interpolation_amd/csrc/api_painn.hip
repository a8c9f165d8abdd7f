// api_painn.hip -- the PaiNN entry points of the C ABI (include/ti_hip.h): creation, the drift family, rollouts, debug taps,
// layout pinning and the per-molecule graph state.
#include "rollout.hpp"

extern "C" {

ti_handle* ti_painn_create(const ti_painn_desc* d, const float* weights, size_t n_weights, const int32_t* edge_src,
                           const int32_t* edge_dst, const int32_t* edge_type, const int32_t* atom_ids, int device)
{
    ti_handle* out = nullptr;
    const int rc = guarded([&]() -> int {
        if (!d || !weights || !atom_ids) return fail(TI_E_ARG, "NULL argument");
        const int F = d->n_features, L = d->n_layers, A = d->n_atoms, E = d->n_edges;
        if (F != 32 && F != 64 && F != 128 && F != 256) return fail(TI_E_UNSUPPORTED, "n_features must be 32, 64, 128 or 256");
        if (L < 1) return fail(TI_E_ARG, "n_layers must be >= 1");
        if (A < 1 || A > 32) return fail(TI_E_UNSUPPORTED, "n_atoms must be in 1..32 (the reference caps it at n_types = 25)");
        if (E < 0 || (E > 0 && (!edge_src || !edge_dst || !edge_type))) return fail(TI_E_ARG, "edge arrays missing");
        if (d->variant < 0 || d->variant > 2) return fail(TI_E_ARG, "unknown variant");
        if (d->n_types < 1) return fail(TI_E_ARG, "n_types must be >= 1");
        if (d->precision != TI_PREC_F32 && d->precision != TI_PREC_F16X2 && d->precision != TI_PREC_F16) return fail(TI_E_ARG, "unknown precision");
        for (int k = 0; k < E; ++k)
            if (edge_src[k] < 0 || edge_src[k] >= A || edge_dst[k] < 0 || edge_dst[k] >= A || edge_type[k] < 0 || edge_type[k] > 3)
                return fail(TI_E_ARG, "edge index / type out of range");
        for (int a = 0; a < A; ++a) if (atom_ids[a] < 0 || atom_ids[a] >= d->n_types) return fail(TI_E_ARG, "atom id out of range");
        std::unique_ptr<ti_handle> h(new_handle(0, device));
        h->d = *d; h->NB = F / 32;
        h->nE = d->variant == TI_VARIANT_AMBIENT ? 4 : d->variant == TI_VARIANT_LATENT_MULTI ? 3 : 2;
        h->ncond = d->variant == TI_VARIANT_AMBIENT ? 2 : d->variant == TI_VARIANT_LATENT_MULTI ? 1 : 0;
        // canonical layout offsets (include/ti_hip.h)
        size_t o = 0;
        h->edge_emb = o; o += 4 * (size_t)F; h->atom_emb = o; o += (size_t)d->n_types * F;
        o = take_mlp(h->embed, o, h->nE * F, F, F);
        h->phi.resize(L); h->w.resize(L); h->upd.resize(L); h->U.resize(L); h->V.resize(L);
        for (int l = 0; l < L; ++l) {
            o = take_mlp(h->phi[l], o, 2 * F, F, 5 * F); o = take_mlp(h->w[l], o, F, F, 5 * F);
            h->U[l] = o; o += (size_t)F * F; h->V[l] = o; o += (size_t)F * F;
            o = take_mlp(h->upd[l], o, 2 * F, F, 3 * F);
        }
        o = take_mlp(h->readout, o, F, F, 2);
        h->Vr = o; o += F;
        if (o != n_weights) return fail(TI_E_ARG, "weight count mismatch: expected " + std::to_string(o) + ", got " + std::to_string(n_weights));
        h->b2_gate = weights[h->readout.b2 + 1];
        // natural-order copy; Vr follows the 2-float readout bias in the canonical layout, so a 16-byte aligned copy of it
        // is appended for the kernels' float4 loads
        std::vector<float> flat(weights, weights + n_weights);
        if (d->precision != TI_PREC_F32)            // the weights' hi halves are plain fp16: refuse what would round to inf
            for (size_t i = 0; i < n_weights; ++i)
                if (!(std::fabs(weights[i]) < 65504.0f))
                    return fail(TI_E_UNSUPPORTED, "precisions f16x2 / f16 need every weight to be finite and below 65504 in magnitude (weight " + std::to_string(i) + ")");
        while (flat.size() % 4) flat.push_back(0.f);
        const size_t vr_aligned = flat.size();
        flat.insert(flat.end(), weights + h->Vr, weights + h->Vr + F);
        h->Vr = vr_aligned;
        h->flat.upload(flat);
        h->atom_ids.upload(std::vector<int32_t>(atom_ids, atom_ids + A));
        build_templates(h.get(), edge_src, edge_dst, edge_type);
        h->has_pair = pair_build_exists(h->NB, 4, d->precision) && build_pair_template(h.get(), edge_src, edge_dst, edge_type);
        select_template(h.get(), 1 << 20);
        pack_painn(h.get(), weights);
        // the update builds that keep v_eff in registers, where the precision and the width have them; triage switch, read like
        // TI_EMBED_CLASSES: TI_UPDATE_KEEP=0 at creation pins the update kernels of before
        h->update_keep_on = update_keep_components(h->NB, d->precision) > 0;
        if (const char* z = std::getenv("TI_UPDATE_KEEP")) if (z[0] == '0') h->update_keep_on = false;
        HIP_CHECK(configure_painn_kernels(h->NB));
        HIP_CHECK(configure_painn_jvp_kernels(h->NB));
        out = h.release();
        return TI_OK;
    });
    return rc == TI_OK ? out : nullptr;
}

// What an evaluation returns beside the drift: nothing, the tangent along one direction, the exact divergence (3A unit seeds), or its
// Hutchinson estimate.  Every mode but the first walks directed edge rows (select_template(.., allow_pair = false)).
enum DriftMode { DRIFT, DRIFT_JVP, DRIFT_DIV, DRIFT_DIV_EST };

// The seven drift-family entry points.  per_mol_t: tv [B] holds one time per molecule (t is unused); xdot / out_tan: DRIFT_JVP;
// out_div: DRIFT_DIV and DRIFT_DIV_EST; n_probes / probe_seed / traj_offset: DRIFT_DIV_EST.
static int painn_drift_impl(ti_handle* h, DriftMode mode, const float* x, const float* xdot, float t, const float* tv, bool per_mol_t,
                            const float* cond, int64_t B, int32_t n_probes, uint64_t probe_seed, int64_t traj_offset, float* out,
                            float* out_tan, float* out_div, int mem)
{
    const bool jvp = mode == DRIFT_JVP, div = mode == DRIFT_DIV || mode == DRIFT_DIV_EST;
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (mode != DRIFT && h->d.precision == TI_PREC_F16) return fail(TI_E_UNSUPPORTED, MSG_NO_FP16_TANGENT);
    if (mode == DRIFT_DIV_EST && n_probes < 1) return fail(TI_E_ARG, "n_probes must be >= 1");
    if (B < 0 || (B > 0 && (!x || (per_mol_t && !tv) || (jvp && (!xdot || !out_tan)) || !out || (div && !out_div) || (h->ncond > 0 && !cond))))
        return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    if (div && h->tap >= 0) return fail(TI_E_ARG, MSG_TAP_ENTRIES);
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B, mode == DRIFT);
        ensure_painn_ws(h, B);
        if (jvp) ensure_jvp_ws(h, B, 1);
        const size_t n = (size_t)B * h->d.n_atoms * 3, nc = (size_t)B * h->d.n_atoms * h->ncond;
        Staged sg(h, mem);
        const float* xd = sg.in(x, h->x, n);
        const float* xdd = jvp ? sg.in(xdot, h->xt, n) : nullptr;
        const float* cd = sg.in(cond, h->cond, nc);
        const float* td = per_mol_t ? sg.in(tv, h->rk_tv, (size_t)B) : nullptr;
        float* od = sg.out(out, h->b1, n);
        float* otd = jvp ? sg.out(out_tan, h->tout, n) : nullptr;
        float* dd = div ? sg.out(out_div, h->divb, (size_t)B) : nullptr;
        phi0_begin_call(h, cd, B, mode == DRIFT && !per_mol_t);      // classes of this call's molecules (the table path of layer 0)
        struct Phi0End { ti_handle* h; ~Phi0End() { phi0_end_call(h); } } phi0_end{h};
        if (mode == DRIFT_DIV_EST) {
            painn_make_probes(h, B, n_probes, probe_seed, traj_offset);
            painn_drift_div_est_dev(h, xd, t, cd, B, n_probes, od, dd, td);
        } else if (mode == DRIFT_DIV) painn_drift_div_dev(h, xd, t, cd, B, od, dd, td);
        else {
            const JvpRun jr{1, xdd, otd};
            painn_drift_dev(h, xd, t, cd, B, od, jvp ? &jr : nullptr, td);
        }
        sg.finish(h->tap < 0);      // a debug tap (refused above for the divergence entries) stops the evaluation early: nothing to copy back
        return TI_OK;
    });
}

int ti_painn_drift(ti_handle* h, const float* x, float t, const float* cond, int64_t B, float* out, int mem)
{
    return painn_drift_impl(h, DRIFT, x, nullptr, t, nullptr, false, cond, B, 0, 0, 0, out, nullptr, nullptr, mem);
}

int ti_painn_drift_tv(ti_handle* h, const float* x, const float* t, const float* cond, int64_t B, float* out, int mem)
{
    return painn_drift_impl(h, DRIFT, x, nullptr, 0.f, t, true, cond, B, 0, 0, 0, out, nullptr, nullptr, mem);
}

int ti_painn_drift_jvp(ti_handle* h, const float* x, const float* xdot, float t, const float* cond, int64_t B, float* out,
                       float* out_tan, int mem)
{
    return painn_drift_impl(h, DRIFT_JVP, x, xdot, t, nullptr, false, cond, B, 0, 0, 0, out, out_tan, nullptr, mem);
}

int ti_painn_drift_div(ti_handle* h, const float* x, float t, const float* cond, int64_t B, float* out, float* out_div, int mem)
{
    return painn_drift_impl(h, DRIFT_DIV, x, nullptr, t, nullptr, false, cond, B, 0, 0, 0, out, nullptr, out_div, mem);
}

int ti_painn_drift_div_tv(ti_handle* h, const float* x, const float* t, const float* cond, int64_t B, float* out, float* out_div, int mem)
{
    return painn_drift_impl(h, DRIFT_DIV, x, nullptr, 0.f, t, true, cond, B, 0, 0, 0, out, nullptr, out_div, mem);
}

int ti_painn_drift_div_est(ti_handle* h, const float* x, float t, const float* cond, int64_t B, int32_t n_probes, uint64_t probe_seed,
                           int64_t traj_offset, float* out, float* out_div, int mem)
{
    return painn_drift_impl(h, DRIFT_DIV_EST, x, nullptr, t, nullptr, false, cond, B, n_probes, probe_seed, traj_offset, out, nullptr, out_div, mem);
}

int ti_painn_drift_div_est_tv(ti_handle* h, const float* x, const float* t, const float* cond, int64_t B, int32_t n_probes,
                              uint64_t probe_seed, int64_t traj_offset, float* out, float* out_div, int mem)
{
    return painn_drift_impl(h, DRIFT_DIV_EST, x, nullptr, 0.f, t, true, cond, B, n_probes, probe_seed, traj_offset, out, nullptr, out_div, mem);
}

// ti_painn_rollout (DRIFT: no second state), ti_painn_rollout_dlogp (DRIFT_DIV: exact divergence) and ti_painn_rollout_dlogp_est
// (DRIFT_DIV_EST: Hutchinson estimate along n_probes probes per trajectory)
static int painn_rollout_impl(ti_handle* h, const ti_rollout_desc* rd, DriftMode mode, int n_probes, uint64_t probe_seed, const float* x0,
                              const float* cond, int64_t B, float div_scale, float out_scale, int reverse_ode, float* out_path,
                              float* out_dlogp, int64_t* n_fevals)
{
    const bool dlogp = mode != DRIFT;
    if (!dlogp) { if (int rc = check_rollout_desc(rd)) return rc; }          // first: needs no handle
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (dlogp) {
        if (h->d.precision == TI_PREC_F16) return fail(TI_E_UNSUPPORTED, MSG_NO_FP16_TANGENT);
        if (mode == DRIFT_DIV_EST && n_probes < 1) return fail(TI_E_ARG, "n_probes must be >= 1");
        if (int rc = check_rollout_desc(rd)) return rc;
        if (rd->scheme == TI_SCHEME_EM) return fail(TI_E_UNSUPPORTED, "dlogp is defined for the deterministic schemes only (EULER, HEUN)");
    }
    if (rd->scheme == TI_SCHEME_DOPRI5_TRAJ && h->obs[1].K > 0) return fail(TI_E_UNSUPPORTED, MSG_TRAJ_OBSERVER);
    if (B < 0 || (B > 0 && (!x0 || !out_path || (dlogp && !out_dlogp) || (h->ncond > 0 && !cond)))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) { if (n_fevals) *n_fevals = 0; return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        select_template(h, B, !dlogp);
        ensure_painn_ws(h, B);
        const int A = h->d.n_atoms;
        const size_t n = (size_t)B * A * 3, nc = (size_t)B * A * h->ncond;
        const hipMemcpyKind in_kind = rd->mem == TI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIP_CHECK(hipMemcpyAsync(h->x.p, x0, n * sizeof(float), in_kind, h->stream));
        const float* cd = cond;
        if (rd->mem == TI_MEM_HOST && nc) { HIP_CHECK(hipMemcpyAsync(h->cond.p, cond, nc * sizeof(float), hipMemcpyHostToDevice, h->stream)); cd = h->cond.p; }
        const int saved_tap = h->tap; h->tap = -1;
        const Ragged rg = ragged_of(h);
        if (mode == DRIFT_DIV_EST) painn_make_probes(h, B, n_probes, probe_seed, rd->traj_offset);
        // cond is constant across a rollout: one class pass for all its steps (TI_SCHEME_DOPRI5_TRAJ evaluates at per-molecule times)
        phi0_begin_call(h, cd, B, !dlogp && rd->scheme != TI_SCHEME_DOPRI5_TRAJ);
        struct Phi0End { ti_handle* h; ~Phi0End() { phi0_end_call(h); } } phi0_end{h};
        DlogpAux aux;
        if (dlogp) {
            aux.dl = h->dl.p; aux.d1 = h->divb.p; aux.d2 = h->div2.p; aux.scaled = h->dlscaled.p; aux.out = out_dlogp;
            aux.n_dl = (size_t)B; aux.div_scale = div_scale; aux.out_scale = out_scale;
        }
        auto eval = [&](const float* xs, float t, const float* tv, float* o, float* dv) {
            if (!dlogp) { painn_drift_dev(h, xs, t, cd, B, o, nullptr, tv); return; }
            if (mode == DRIFT_DIV_EST) painn_drift_div_est_dev(h, xs, t, cd, B, n_probes, o, dv, tv);
            else painn_drift_div_dev(h, xs, t, cd, B, o, dv, tv);
            if (reverse_ode) {      // (-b, +div): ode_wrapper.py:49
                HIP_CHECK(launch_scale(o, o, -1.0f, (long long)n, h->stream));
                HIP_CHECK(launch_scale(dv, dv, -1.0f, (long long)B, h->stream));
            }
        };
        auto drift = [&](const float* xs, float t, float* o, float* dv) { eval(xs, t, nullptr, o, dv); };
        auto drift_tv = [&](const float* xs, const float* tv, float* o, float* dv) { eval(xs, 0.f, tv, o, dv); };
        const int rc = rd->scheme == TI_SCHEME_DOPRI5_TRAJ ? rollout_rk_traj(h, rd, h->x.p, B, A * 3, out_path, n_fevals, drift_tv, aux, rg)
                     : rd->scheme >= TI_SCHEME_DOPRI5 ? rollout_rk(h, rd, h->x.p, n, out_path, n_fevals, drift, aux, rg)
                                                      : rollout_common(h, rd, h->x.p, h->b1.p, h->b2.p, h->xt.p, n, B, A * 3, A, out_path, n_fevals, drift, aux, rg);
        h->tap = saved_tap;
        return rc;
    });
}

int ti_painn_rollout(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* cond, int64_t B, float* out_path,
                     int64_t* n_fevals)
{
    return painn_rollout_impl(h, rd, DRIFT, 0, 0, x0, cond, B, 0.f, 0.f, 0, out_path, nullptr, n_fevals);
}

int ti_painn_rollout_dlogp(ti_handle* h, const ti_rollout_desc* rd, const float* x0, const float* cond, int64_t B, float div_scale,
                           float out_scale, int reverse_ode, float* out_path, float* out_dlogp, int64_t* n_fevals)
{
    return painn_rollout_impl(h, rd, DRIFT_DIV, 0, 0, x0, cond, B, div_scale, out_scale, reverse_ode, out_path, out_dlogp, n_fevals);
}

int ti_painn_rollout_dlogp_est(ti_handle* h, const ti_rollout_desc* rd, int32_t n_probes, uint64_t probe_seed, const float* x0,
                               const float* cond, int64_t B, float div_scale, float out_scale, int reverse_ode, float* out_path,
                               float* out_dlogp, int64_t* n_fevals)
{
    return painn_rollout_impl(h, rd, DRIFT_DIV_EST, n_probes, probe_seed, x0, cond, B, div_scale, out_scale, reverse_ode, out_path, out_dlogp, n_fevals);
}

int ti_painn_debug_tap(ti_handle* h, int stage)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->d.precision == TI_PREC_F16 && stage >= 0) return fail(TI_E_UNSUPPORTED, "debug taps read fp32 state; not available in the fp16 storage mode");
    h->tap = stage;
    return TI_OK;
}

int ti_painn_debug_phi0_path(ti_handle* h, int32_t* n_classes)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (n_classes) *n_classes = h->phi0_found;
    return h->phi0_last;
}

int ti_painn_debug_pair_blocks(ti_handle* h, int32_t* G, int32_t* nblk, int32_t* n_tile)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (!h->has_pair) return 0;
    if (G) *G = h->tpl[2].G;
    if (nblk) *nblk = h->tpl[2].nblk;
    if (n_tile) *n_tile = h->tpl[2].n_tile;
    return 1;
}

int ti_painn_debug_pair_seeded(ti_handle* h, int32_t* template_seeded)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (template_seeded) *template_seeded = h->has_pair && h->pair_seeded ? 1 : 0;
    return h->seeded_last;
}

int ti_painn_debug_pair_tails(ti_handle* h, int32_t* groups_per_wave)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (groups_per_wave) *groups_per_wave = h->has_pair ? h->pair_tail_S : 0;
    return h->tails_last;
}

int ti_painn_debug_embed_path(ti_handle* h)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    return h->embed_cls_last;
}

int ti_painn_debug_update_keep(ti_handle* h)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    return h->update_keep_last;
}

int ti_painn_debug_poison(ti_handle* h, int64_t B, float value)
{
    if (!h || h->kind != 0 || B <= 0) return fail(TI_E_ARG, "not a painn handle / B");
    return guarded([&]() -> int {
        set_device(h);
        ensure_painn_ws(h, B);
        const size_t N = (size_t)B * h->d.n_atoms, F = h->d.n_features;
        const unsigned bits = __builtin_bit_cast(unsigned, value);
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->dsacc.p, (int)bits, N * F, h->stream));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->dvacc.p, (int)bits, N * 3 * F, h->stream));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->cacc.p, (int)bits, N * 3 * F, h->stream));
        // the edge state and the parked geometry as well: every row a launch reads was written earlier in the same evaluation, and the
        // rows the pair-major kernel skips (pairs that do not exist) are never read
        static_assert(sizeof(*h->e.p) == 4 && sizeof(*h->enc.p) == 4 && sizeof(*h->geo.p) == 4, "32-bit fills");
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->e.p, (int)bits, h->e.n, h->stream));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->enc.p, (int)bits, h->enc.n, h->stream));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->geo.p, (int)bits, h->geo.n, h->stream));
        // the layer-0 phi table too: every entry an evaluation reads was written by its own table launch
        if (h->phi0_tab.n) HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->phi0_tab.p, (int)bits, h->phi0_tab.n, h->stream));
        // s and P, and their per-class twins: an evaluation whose embed launch covers the classes alone must not read the full rows
        // before layer 0's update has written them (every other evaluation's embed launch replaces them first)
        static_assert(sizeof(*h->s.p) == 4 && sizeof(*h->P.p) == 4, "32-bit fills");
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->s.p, (int)bits, h->s.n, h->stream));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->P.p, (int)bits, h->P.n, h->stream));
        if (h->s_cls.n) HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->s_cls.p, (int)bits, h->s_cls.n, h->stream));
        if (h->P_cls.n) HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)h->P_cls.p, (int)bits, h->P_cls.n, h->stream));
        return TI_OK;
    });
}

int ti_painn_debug_read(ti_handle* h, int what, float* out, size_t n_floats)
{
    if (!h || h->kind != 0 || !out) return fail(TI_E_ARG, "bad argument");
    return guarded([&]() -> int {
        set_device(h);
        const size_t A = h->d.n_atoms, F = h->d.n_features, E = h->d.n_edges, B = (size_t)h->last_B, N = B * A;
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (what == 0) {
            if (n_floats != N * F) return fail(TI_E_ARG, "size mismatch (s)");
            std::vector<float> ds(n_floats);                  // pending invariant messages (zero after an update stage)
            HIP_CHECK(hipMemcpy(out, h->s.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(ds.data(), h->dsacc.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n_floats; ++i) out[i] += ds[i];
        } else if (what == 1) {
            // v as the reference sees it at the tap: v + dvacc + cacc x v (the accumulators are zero after an update stage)
            if (n_floats != N * 3 * F) return fail(TI_E_ARG, "size mismatch (v)");
            std::vector<float> v(n_floats), dv(n_floats), cc(n_floats);
            HIP_CHECK(hipMemcpy(v.data(), h->v.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(dv.data(), h->dvacc.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(cc.data(), h->cacc.p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t nd = 0; nd < N; ++nd)
                for (size_t f = 0; f < F; ++f)
                    for (int c = 0; c < 3; ++c) {
                        const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                        auto at = [&](const std::vector<float>& a, int cc2) { return a[(nd * 3 + cc2) * F + f]; };
                        out[(nd * 3 + c) * F + f] = (at(v, c) + at(dv, c)) + (at(cc, c1) * at(v, c2) - at(cc, c2) * at(v, c1));
                    }
        } else if (what == 2) {
            if (n_floats != B * E * F) return fail(TI_E_ARG, "size mismatch (e)");
            const size_t RB = ti::EDGE_ROWS_PER_BLOCK, rows = (B + h->G - 1) / h->G * h->parts * h->nblk * RB * (h->active == 2 ? 2 : 1);
            std::vector<float> e(rows * F);
            HIP_CHECK(hipMemcpy(e.data(), h->e.p, e.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t m = 0; m < B; ++m)
                for (size_t k = 0; k < E; ++k)                                   // k = sorted position
                    std::memcpy(out + (m * E + h->perm[k]) * F, e.data() + edge_row_of(h, m, k) * F, F * sizeof(float));
        } else if (what >= 3 && what <= 5) {
            // tangents of the last ti_painn_drift_jvp call (one direction per molecule), composed like their primal twins
            if (h->last_D != 1 || (size_t)h->last_VB != B) return fail(TI_E_ARG, "tangent taps need a preceding ti_painn_drift_jvp call");
            auto fetch = [&](const DevBuf<float>& b, size_t n) { std::vector<float> v(n); HIP_CHECK(hipMemcpy(v.data(), b.p, n * sizeof(float), hipMemcpyDeviceToHost)); return v; };
            if (what == 3) {
                if (n_floats != N * F) return fail(TI_E_ARG, "size mismatch (ts)");
                const auto ts = fetch(h->ts, n_floats), td = fetch(h->tdsacc, n_floats);
                for (size_t i = 0; i < n_floats; ++i) out[i] = ts[i] + td[i];
            } else if (what == 4) {
                if (n_floats != N * 3 * F) return fail(TI_E_ARG, "size mismatch (tv)");
                const auto v = fetch(h->v, n_floats), cc = fetch(h->cacc, n_floats);
                const auto tv = fetch(h->tv, n_floats), tdv = fetch(h->tdvacc, n_floats), tcc = fetch(h->tcacc, n_floats);
                for (size_t nd = 0; nd < N; ++nd)
                    for (size_t f = 0; f < F; ++f)
                        for (int c = 0; c < 3; ++c) {
                            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                            auto at = [&](const std::vector<float>& a, int cc2) { return a[(nd * 3 + cc2) * F + f]; };
                            out[(nd * 3 + c) * F + f] = (at(tv, c) + at(tdv, c)) + ((at(tcc, c1) * at(v, c2) + at(cc, c1) * at(tv, c2)) -
                                                                                     (at(tcc, c2) * at(v, c1) + at(cc, c2) * at(tv, c1)));
                        }
            } else {
                if (n_floats != B * E * F) return fail(TI_E_ARG, "size mismatch (te)");
                const size_t RB = ti::EDGE_ROWS_PER_BLOCK, rows = (B + h->G - 1) / h->G * h->parts * h->nblk * RB;
                const auto e = fetch(h->te, rows * F);
                for (size_t m = 0; m < B; ++m)
                    for (size_t k = 0; k < E; ++k)
                        std::memcpy(out + (m * E + h->perm[k]) * F, e.data() + edge_row_of(h, m, k) * F, F * sizeof(float));
            }
        } else return fail(TI_E_ARG, "unknown tap");
        return TI_OK;
    });
}

// ------------------------------------------------------------------------------------------- layouts, graph state
int ti_painn_set_template(ti_handle* h, int which)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (which != TI_TEMPLATE_AUTO && which != TI_TEMPLATE_THROUGHPUT && which != TI_TEMPLATE_LATENCY && which != TI_TEMPLATE_PAIR) return fail(TI_E_ARG, "unknown template");
    if (which == TI_TEMPLATE_LATENCY && h->n_tpl < 2) which = TI_TEMPLATE_THROUGHPUT;      // this species has only one layout
    if (which == TI_TEMPLATE_PAIR && !h->has_pair) which = TI_TEMPLATE_THROUGHPUT;         // no pair-major layout for this graph / width / precision
    h->pinned_tpl = which;
    return TI_OK;
}

int ti_painn_template_for(ti_handle* h, int64_t B)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (h->has_pair && mask_blocks_pair(h) && pinned_template(h) == TI_TEMPLATE_PAIR)
        return fail(TI_E_UNSUPPORTED, "the pair layout is pinned, and the edge mask in force is not symmetric for every molecule");
    return template_for(h, B);
}

int ti_painn_set_edge_mask(ti_handle* h, const uint32_t* mask, int64_t B, int mem)
{
    // the arguments first, then the handle: each refusal has its own message, checkable without a device
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (mask && B < 1) return fail(TI_E_ARG, "B < 1");
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (!mask) { clear_graph_state(h); return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        const int A = h->d.n_atoms;
        std::vector<uint32_t> m((size_t)B * A);
        if (mem == TI_MEM_DEVICE) HIP_CHECK(hipMemcpy(m.data(), mask, m.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        else std::memcpy(m.data(), mask, m.size() * sizeof(uint32_t));
        std::vector<int32_t> none; std::vector<uint8_t> no_types;
        return set_graph_state(h, m, none, no_types, B);
    });
}

int ti_painn_set_molecules(ti_handle* h, const int32_t* n_atoms, const uint32_t* mask, const uint8_t* pair_type, int64_t B, int mem)
{
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (n_atoms && B < 1) return fail(TI_E_ARG, "B < 1");
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (!n_atoms) { clear_graph_state(h); return TI_OK; }
    return guarded([&]() -> int {
        set_device(h);
        const int A = h->d.n_atoms;
        auto fetch = [&](void* dst, const void* src, size_t bytes) {
            if (mem == TI_MEM_DEVICE) HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            else std::memcpy(dst, src, bytes);
        };
        std::vector<int32_t> na((size_t)B);
        fetch(na.data(), n_atoms, na.size() * sizeof(int32_t));
        for (long long b = 0; b < B; ++b)
            if (na[b] < 1 || na[b] > A) return fail(TI_E_ARG, "n_atoms[" + std::to_string(b) + "] = " + std::to_string(na[b]) + " is outside 1.." + std::to_string(A));
        std::vector<uint8_t> pt;
        if (pair_type) {
            pt.resize((size_t)B * A * A);
            fetch(pt.data(), pair_type, pt.size());
            for (size_t i = 0; i < pt.size(); ++i) if (pt[i] > 3) return fail(TI_E_ARG, "pair_type above 3 (molecule " + std::to_string(i / ((size_t)A * A)) + ")");
        }
        std::vector<uint32_t> m((size_t)B * A, 0xffffffffu);       // NULL: every template edge (between real atoms, set_graph_state)
        if (mask) fetch(m.data(), mask, m.size() * sizeof(uint32_t));
        return set_graph_state(h, m, na, pt, B);
    });
}

}  // extern "C"
