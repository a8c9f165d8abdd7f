// api_ff.hip -- C ABI of the force field (include/ti_hip.h): its tables and energies (ti_obs_ff_set, ti_obs_ff_energy), its forces
// (ti_obs_ff_forces), Langevin dynamics with them (ti_obs_ff_set_masses, ti_obs_ff_langevin) and replica exchange between its launches
// (ti_obs_ff_remd): checks, staging and the launch cut.  Kernels: obs_ff_kernels.hip, obs_ff_md_kernels.hip, obs_ff_remd_kernels.hip.
#include "ti_handle.hpp"
#include "ff_device.hpp"

// the packed incidence list of the bonded term words (bonds, angles, torsions of lengths n[0..2]; ff_device.hpp)
static std::vector<int32_t> ff_build_incidence(const std::vector<int32_t>& words, const int* n, int A)
{
    const int chunks = ff_chunks(n[0]) + ff_chunks(n[1]) + ff_chunks(n[2]);
    std::vector<uint16_t> off((size_t)chunks * A + 1, 0);
    std::vector<uint8_t> entries;
    int q = 0, first = 0;
    for (int t = 0; t < 3; first += n[t], ++t)
        for (int base = 0; base < n[t]; base += FF_CHUNK, ++q)
            for (int a = 0; a < A; ++a) {
                off[(size_t)q * A + a] = (uint16_t)entries.size();
                for (int l = 0; l < FF_CHUNK && base + l < n[t]; ++l)              // ascending term, then slot
                    for (int s = 0; s < 2 + t; ++s)
                        if (ff_atom(words[first + base + l], s) == a) entries.push_back((uint8_t)(l << 2 | s));
            }
    off[(size_t)chunks * A] = (uint16_t)entries.size();
    std::vector<int32_t> out((size_t)FF_INC_OFF_WORDS + (entries.size() + 3) / 4, 0);
    std::memcpy(out.data(), off.data(), off.size() * sizeof(uint16_t));
    if (!entries.empty()) std::memcpy(out.data() + FF_INC_OFF_WORDS, entries.data(), entries.size());
    return out;
}

static FfTablesDev ff_tables(const ti_handle* h)
{
    FfTablesDev t{};
    t.A = h->d.n_atoms; t.nb = h->ff_n[0]; t.na = h->ff_n[1]; t.nt = h->ff_n[2]; t.np = h->ff_n[3];
    t.coulomb = h->ff_coulomb; t.idx = h->ff_idx.p; t.par = h->ff_par.p; t.inc = h->ff_inc.p; t.inc_words = (int)h->ff_inc.n;
    return t;
}

// The refusal of a call with per-molecule temperatures T_dev [B], before anything is written: one launch and one wait, the index
// found as ti_obs_weights finds its own
static int ff_temperature_refusal(ti_handle* h, const float* T_dev, long long B)
{
    hipStream_t st = h->stream;
    obs_scratch(h);
    double bad = 0.0;
    HIP_CHECK(launch_obs_ff_bad_temperature(h->obs_red.p, T_dev, B, st));
    HIP_CHECK(hipMemcpyAsync(&bad, h->obs_red.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (bad < (double)B) return fail(TI_E_ARG, "T must be finite and > 0: index " + std::to_string((long long)bad));
    return TI_OK;
}

int ti_obs_ff_set(ti_handle* h, const ti_ff_desc* desc, const int32_t* bond_idx, const double* bond_par, const int32_t* angle_idx,
                  const double* angle_par, const int32_t* torsion_idx, const double* torsion_par, const double* pair_par)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (!desc) { h->ff_on = false; h->ff_mass_on = false; return TI_OK; }
    if (!h->natoms.empty()) return fail(TI_E_UNSUPPORTED, "one force field is one species: clear ti_painn_set_molecules first");
    const int A = h->d.n_atoms;
    const int n[4] = {desc->n_bonds, desc->n_angles, desc->n_torsions, desc->n_pairs};
    const int cap[4] = {TI_FF_MAX_BONDS, TI_FF_MAX_ANGLES, TI_FF_MAX_TORSIONS, TI_FF_MAX_PAIRS};
    const char* name[4] = {"bond", "angle", "torsion", "pair"};
    const int32_t* idx[3] = {bond_idx, angle_idx, torsion_idx};
    const double* par[4] = {bond_par, angle_par, torsion_par, pair_par};
    for (int t = 0; t < 4; ++t) {
        if (n[t] < 0 || n[t] > cap[t]) return fail(TI_E_ARG, std::string(name[t]) + " count " + std::to_string(n[t]) + " is outside 0.." + std::to_string(cap[t]));
        if (n[t] > 0 && (!par[t] || (t < 3 && !idx[t]))) return fail(TI_E_ARG, std::string(name[t]) + " table is NULL");
    }
    if (n[3] != A * (A - 1) / 2) return fail(TI_E_ARG, "the pair table must hold all A (A - 1) / 2 = " + std::to_string(A * (A - 1) / 2) + " pairs, got " + std::to_string(n[3]));
    if (!std::isfinite(desc->coulomb)) return fail(TI_E_ARG, "coulomb must be finite");
    std::vector<int32_t> words; std::vector<double> pars;
    for (int t = 0; t < 3; ++t) {                              // bonds (2 atoms, 2 parameters), angles (3, 2), torsions (4, 3)
        const int na = 2 + t, np = t == 2 ? 3 : 2;
        for (int k = 0; k < n[t]; ++k) {
            const std::string what = std::string(name[t]) + " " + std::to_string(k);
            const int32_t* a = idx[t] + (size_t)na * k;
            const double* q = par[t] + (size_t)np * k;
            int32_t w = 0;
            for (int s = 0; s < na; ++s) {
                if (a[s] < 0 || a[s] >= A) return fail(TI_E_ARG, what + ": atom index outside 0.." + std::to_string(A - 1));
                for (int s2 = 0; s2 < s; ++s2)
                    if (a[s2] == a[s]) return fail(TI_E_ARG, what + ": atom " + std::to_string(a[s]) + " is repeated");
                w |= a[s] << (5 * s);
            }
            for (int s = 0; s < np; ++s)
                if (!std::isfinite(q[s])) return fail(TI_E_ARG, what + ": non-finite parameter");
            if (t == 2) {                                      // (n, phase, k): the periodicity goes into the word
                if (q[0] != std::floor(q[0]) || q[0] < 1.0 || q[0] > 6.0) return fail(TI_E_ARG, what + ": the periodicity must be an integer in 1..6");
                w |= (int32_t)q[0] << 20;
                pars.push_back(q[1]); pars.push_back(q[2]);
            } else {
                pars.push_back(q[0]); pars.push_back(q[1]);
            }
            words.push_back(w);
        }
    }
    for (int i = 0, k = 0; i < A; ++i)                         // row i (2A - i - 1) / 2 + (j - i - 1)
        for (int j = i + 1; j < A; ++j, ++k) {
            const double* q = pair_par + 3 * (size_t)k;
            const std::string what = "pair " + std::to_string(k) + " (" + std::to_string(i) + ", " + std::to_string(j) + ")";
            if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) return fail(TI_E_ARG, what + ": non-finite parameter");
            if (q[1] < 0.0 || q[2] < 0.0) return fail(TI_E_ARG, what + ": sigma and eps must be >= 0");
            words.push_back(i | j << 5 | ((q[0] != 0.0 || q[2] != 0.0) ? FF_LIVE : 0));
            pars.insert(pars.end(), q, q + 3);
        }
    const std::vector<int32_t> inc = ff_build_incidence(words, n, A);      // of the bonded terms, for ti_obs_ff_forces / ti_obs_ff_langevin
    return guarded([&]() -> int {
        set_device(h);
        h->ff_on = false;
        h->ff_mass_on = false;                                 // the masses go with the force field (ti_obs_ff_set_masses)
        h->ff_idx.upload(words);
        h->ff_par.upload(pars);
        h->ff_inc.upload(inc);
        std::copy(n, n + 4, h->ff_n);
        h->ff_coulomb = desc->coulomb;
        h->ff_on = true;
        return TI_OK;
    });
}

// the refusals of ti_obs_ff_energy and ti_obs_ff_forces, in the header's order; out: the output the call cannot do without
static int ff_eval_refusal(const ti_handle* h, const float* x, const double* out, int64_t B, double to_nm, int mem)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (B < 0 || (B > 0 && (!x || !out))) return fail(TI_E_ARG, "NULL buffer");
    if (!std::isfinite(to_nm)) return fail(TI_E_ARG, "to_nm must be finite");
    if (!h->ff_on) return fail(TI_E_ARG, "no force field set (ti_obs_ff_set)");
    if (!h->natoms.empty()) return fail(TI_E_UNSUPPORTED, "one force field is one species: clear ti_painn_set_molecules first");
    return TI_OK;
}

int ti_obs_ff_energy(ti_handle* h, const float* x, int64_t B, double to_nm, const float* T, double* out_e, double* out_terms, int mem)
{
    if (int rc = ff_eval_refusal(h, x, out_e, B, to_nm, mem)) return rc;
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const int A = h->d.n_atoms;
        Staged sg(h, mem);
        const float* xd = sg.in(x, h->obs_x, (size_t)B * 3 * A);
        const float* Td = T ? sg.in(T, h->ff_T, (size_t)B) : nullptr;
        if (Td) { if (int rc = ff_temperature_refusal(h, Td, B)) return rc; }
        FfParams p{};
        p.x = xd; p.T = Td; p.B = B; p.A = A; p.to_nm = to_nm; p.coulomb = h->ff_coulomb;
        p.nb = h->ff_n[0]; p.na = h->ff_n[1]; p.nt = h->ff_n[2]; p.np = h->ff_n[3];
        p.idx = h->ff_idx.p; p.par = h->ff_par.p;
        p.e = sg.out(out_e, h->ff_e, (size_t)B);
        p.terms = out_terms ? sg.out(out_terms, h->ff_terms, (size_t)B * 4) : nullptr;
        HIP_CHECK(launch_obs_ff_energy(p, st));
        sg.finish();
        return TI_OK;
    });
}

int ti_obs_ff_forces(ti_handle* h, const float* x, int64_t B, double to_nm, const float* T, double* out_f, double* out_e, int mem)
{
    if (int rc = ff_eval_refusal(h, x, out_f, B, to_nm, mem)) return rc;
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const int A = h->d.n_atoms;
        Staged sg(h, mem);
        const float* xd = sg.in(x, h->obs_x, (size_t)B * 3 * A);
        const float* Td = T ? sg.in(T, h->ff_T, (size_t)B) : nullptr;
        if (Td) { if (int rc = ff_temperature_refusal(h, Td, B)) return rc; }
        FfForceParams p{};
        p.t = ff_tables(h);
        p.x = xd; p.T = Td; p.B = B; p.to_nm = to_nm;
        p.f = sg.out(out_f, h->ff_f, (size_t)B * 3 * A);
        p.e = out_e ? sg.out(out_e, h->ff_e, (size_t)B) : nullptr;
        HIP_CHECK(launch_obs_ff_forces(p, st));
        sg.finish();
        return TI_OK;
    });
}

int ti_obs_ff_set_masses(ti_handle* h, const double* m)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (!m) { h->ff_mass_on = false; return TI_OK; }
    if (!h->ff_on) return fail(TI_E_ARG, "no force field set (ti_obs_ff_set): the masses go with it");
    const int A = h->d.n_atoms;
    for (int a = 0; a < A; ++a)
        if (!(std::isfinite(m[a]) && m[a] > 0.0)) return fail(TI_E_ARG, "mass " + std::to_string(a) + " must be finite and > 0");
    return guarded([&]() -> int {
        set_device(h);
        h->ff_mass_on = false;
        h->ff_mass.upload(std::vector<double>(m, m + A));
        h->ff_mass_on = true;
        return TI_OK;
    });
}

// The refusals of ti_obs_ff_langevin that need no device, in the header's order; ti_obs_ff_remd gives them first
static int md_refusal(const ti_handle* h, const ti_md_desc* d, const double* pos, const double* vel, const float* T, int64_t B, double to_nm,
                      const float* out_frames, const double* out_epot, const double* out_ekin, int mem)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    if (!d || !pos || !T) return fail(TI_E_ARG, "NULL desc, pos or T");
    if (!vel && !d->draw_velocities) return fail(TI_E_ARG, "vel is NULL and draw_velocities is off");
    if (!(std::isfinite(d->dt) && d->dt > 0.0)) return fail(TI_E_ARG, "dt must be finite and > 0");
    if (!(std::isfinite(d->friction) && d->friction >= 0.0)) return fail(TI_E_ARG, "friction must be finite and >= 0");
    if (d->n_steps < 0 || d->stride < 0 || d->step_offset < 0 || d->steps_per_launch < 0) return fail(TI_E_ARG, "a negative count");
    if (d->stride > 0 && !out_frames && !out_epot && !out_ekin) return fail(TI_E_ARG, "stride > 0 needs out_frames, out_epot or out_ekin");
    if (B < 1) return fail(TI_E_ARG, "B < 1");
    if (!(std::isfinite(to_nm) && to_nm != 0.0)) return fail(TI_E_ARG, "to_nm must be finite and not 0");
    if (!h->ff_on) return fail(TI_E_ARG, "no force field set (ti_obs_ff_set)");
    if (!h->ff_mass_on) return fail(TI_E_ARG, "no masses set (ti_obs_ff_set_masses)");
    if (!h->natoms.empty()) return fail(TI_E_UNSUPPORTED, "one force field is one species: clear ti_painn_set_molecules first");
    return TI_OK;
}

// what replica exchange adds to a Langevin call (r == NULL: none of it)
struct RemdArgs {
    const ti_remd_desc* r; const int64_t* ladder_ids; int32_t* walker; int32_t* out_walker; int64_t* out_counts;
};

// The body of ti_obs_ff_langevin and ti_obs_ff_remd: the Langevin launches of the call, cut after every steps_per_launch steps and,
// with x.r, at every exchange attempt, which is one launch of its own between two of them
static int md_run(ti_handle* h, const ti_md_desc* d, const RemdArgs& x, double* pos, double* vel, const float* T, const int64_t* ids, int64_t B,
                  double to_nm, float* out_frames, double* out_epot, double* out_ekin, int mem)
{
    return guarded([&]() -> int {
        set_device(h);
        hipStream_t st = h->stream;
        const int A = h->d.n_atoms;
        const size_t n_state = (size_t)B * 3 * A;
        const long long n_frames = d->stride > 0 ? d->n_steps / d->stride : 0;
        const bool host = mem == TI_MEM_HOST;
        Staged sg(h, mem);
        const float* Td = sg.in(T, h->ff_T, (size_t)B);
        const int64_t* idd = ids ? sg.in(ids, h->md_ids, (size_t)B) : nullptr;
        // the state is advanced in a working copy: pos / vel change only when the whole call succeeds
        grow(h->md_pos, n_state); grow(h->md_vel, n_state); grow(h->md_flag, (size_t)B + 2); obs_scratch(h);
        HIP_CHECK(hipMemcpyAsync(h->md_pos.p, pos, n_state * sizeof(double), in_kind(mem), st));
        if (!d->draw_velocities) HIP_CHECK(hipMemcpyAsync(h->md_vel.p, vel, n_state * sizeof(double), in_kind(mem), st));
        HIP_CHECK(hipMemsetAsync(h->md_flag.p, 0, (size_t)B * sizeof(int), st));
        // not ff_temperature_refusal: the launches below read the flag and return at once on a bad T, the host waits once, at the end
        HIP_CHECK(launch_obs_ff_bad_temperature(h->obs_red.p, Td, B, st));
        MdParams p{};
        p.t = ff_tables(h);
        p.pos = h->md_pos.p; p.vel = h->md_vel.p; p.T = Td; p.ids = reinterpret_cast<const long long*>(idd); p.mass = h->ff_mass.p;
        p.B = B; p.traj_offset = d->traj_offset; p.dt = d->dt; p.a = d->friction > 0.0 ? std::exp(-d->friction * d->dt) : 1.0; p.to_nm = to_nm;
        p.stride = d->stride; p.n_frames = n_frames; p.seed = d->seed; p.bad_T = h->obs_red.p; p.flag = h->md_flag.p;
        p.frames = out_frames && n_frames ? sg.out(out_frames, h->md_frames, (size_t)B * n_frames * 3 * A) : nullptr;
        p.epot = out_epot && n_frames ? sg.out(out_epot, h->md_epot, (size_t)B * n_frames) : nullptr;
        p.ekin = out_ekin && n_frames ? sg.out(out_ekin, h->md_ekin, (size_t)B * n_frames) : nullptr;
        // replica exchange: the labels advance in a working copy too; the history and the counts of a host call are staged
        const long long every = x.r ? x.r->exchange_every : 0;
        const long long n_attempts = x.r ? (d->step_offset + d->n_steps) / every - d->step_offset / every : 0;
        const size_t n_counts = x.r ? (size_t)(B / x.r->n_rungs) * (x.r->n_rungs - 1) * 2 : 0;
        RemdParams q{};
        int32_t* hist = nullptr;
        if (x.r) {
            grow(h->md_walker, (size_t)B);
            const int32_t* win = x.walker && host ? sg.in(x.walker, h->md_walker_in, (size_t)B) : x.walker;
            HIP_CHECK(launch_obs_ff_remd_walker(h->md_walker.p, win, B, x.r->n_rungs, h->obs_red.p, st));      // behind the T check
            q.t = p.t; q.pos = p.pos; q.vel = p.vel; q.T = Td; q.B = B; q.K = x.r->n_rungs; q.seed = d->seed; q.mass = h->ff_mass.p; q.dt = d->dt;
            q.ladder_ids = reinterpret_cast<const long long*>(x.ladder_ids ? sg.in(x.ladder_ids, h->md_ladder_ids, (size_t)(B / x.r->n_rungs)) : nullptr);
            q.walker = h->md_walker.p; q.flag = h->md_flag.p; q.bad_T = h->obs_red.p;
            if (x.out_walker && n_attempts) {
                if (host) grow(h->md_out_walker, (size_t)n_attempts * B);
                hist = host ? h->md_out_walker.p : x.out_walker;
            }
            if (x.out_counts) {
                if (host) grow(h->md_counts, n_counts);
                q.counts = reinterpret_cast<long long*>(host ? h->md_counts.p : x.out_counts);
                HIP_CHECK(hipMemsetAsync(q.counts, 0, n_counts * sizeof(int64_t), st));
            }
        }
        const long long per = d->steps_per_launch > 0 ? d->steps_per_launch : TI_MD_DEFAULT_STEPS_PER_LAUNCH;
        long long done = 0, attempts = 0;
        for (int launch = 0; launch == 0 || done < d->n_steps; ++launch) {      // n_steps = 0: one launch (it may draw the velocities)
            p.n_steps = std::min<long long>(per, d->n_steps - done);
            const long long g = d->step_offset + done;                          // steps behind the state, over all chained calls
            if (x.r) p.n_steps = std::min<long long>(p.n_steps, (g / every + 1) * every - g);
            p.steps_before = done; p.step0 = g; p.launch = launch; p.draw = launch == 0 && d->draw_velocities;
            HIP_CHECK(launch_obs_ff_langevin(p, st));
            done += p.n_steps;
            if (x.r && p.n_steps > 0 && (g + p.n_steps) % every == 0) {         // a frame due here is written: it shows the state before
                q.attempt = (g + p.n_steps) / every;
                q.out_walker = hist ? hist + (size_t)attempts * B : nullptr;
                HIP_CHECK(launch_obs_ff_remd(q, st));
                ++attempts;
            }
        }
        std::vector<int> flag((size_t)B);
        double bad = 0.0;
        HIP_CHECK(hipMemcpyAsync(&bad, h->obs_red.p, sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(flag.data(), h->md_flag.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));           // the one wait of the call that does not move results
        if (bad < 0.0) return fail(TI_E_ARG, "walker must lie in 0 .. n_rungs - 1: index " + std::to_string((long long)(-1.0 - bad)));
        if (bad < (double)B) return fail(TI_E_ARG, "T must be finite and > 0: index " + std::to_string((long long)bad));
        for (int64_t b = 0; b < B; ++b)
            if (flag[b])
                return fail(TI_E_NAN, "replica " + std::to_string((long long)b) + ": the state turned non-finite in launch " + std::to_string(flag[b] - 1) +
                                          " (pos and vel are left as they were)");
        HIP_CHECK(hipMemcpyAsync(pos, h->md_pos.p, n_state * sizeof(double), out_kind(mem), st));
        if (vel) HIP_CHECK(hipMemcpyAsync(vel, h->md_vel.p, n_state * sizeof(double), out_kind(mem), st));
        if (x.r && x.walker) HIP_CHECK(hipMemcpyAsync(x.walker, h->md_walker.p, (size_t)B * sizeof(int32_t), out_kind(mem), st));
        if (hist && host) HIP_CHECK(hipMemcpyAsync(x.out_walker, hist, (size_t)n_attempts * B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (q.counts && host) HIP_CHECK(hipMemcpyAsync(x.out_counts, q.counts, n_counts * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        sg.finish();
        return TI_OK;
    });
}

int ti_obs_ff_langevin(ti_handle* h, const ti_md_desc* d, double* pos, double* vel, const float* T, const int64_t* ids, int64_t B,
                       double to_nm, float* out_frames, double* out_epot, double* out_ekin, int mem)
{
    if (int rc = md_refusal(h, d, pos, vel, T, B, to_nm, out_frames, out_epot, out_ekin, mem)) return rc;
    return md_run(h, d, RemdArgs{}, pos, vel, T, ids, B, to_nm, out_frames, out_epot, out_ekin, mem);
}

int ti_obs_ff_remd(ti_handle* h, const ti_md_desc* d, const ti_remd_desc* r, double* pos, double* vel, const float* T, const int64_t* ids,
                   const int64_t* ladder_ids, int64_t B, double to_nm, int32_t* walker, float* out_frames, double* out_epot, double* out_ekin,
                   int32_t* out_walker, int64_t* out_counts, int mem)
{
    if (int rc = md_refusal(h, d, pos, vel, T, B, to_nm, out_frames, out_epot, out_ekin, mem)) return rc;
    if (!r) return fail(TI_E_ARG, "NULL remd desc");
    if (r->n_rungs < 2 || r->n_rungs > TI_REMD_MAX_RUNGS) return fail(TI_E_ARG, "n_rungs must lie in 2 .. " + std::to_string(TI_REMD_MAX_RUNGS));
    if (B % r->n_rungs != 0) return fail(TI_E_ARG, "B must be a multiple of n_rungs");
    if (r->exchange_every < 1) return fail(TI_E_ARG, "exchange_every < 1");
    if (r->reserved != 0) return fail(TI_E_ARG, "reserved must be 0");
    if (walker && mem == TI_MEM_HOST)
        for (int64_t b = 0; b < B; ++b)
            if (walker[b] < 0 || walker[b] >= r->n_rungs) return fail(TI_E_ARG, "walker must lie in 0 .. n_rungs - 1: index " + std::to_string((long long)b));
    return md_run(h, d, RemdArgs{r, ladder_ids, walker, out_walker, out_counts}, pos, vel, T, ids, B, to_nm, out_frames, out_epot, out_ekin, mem);
}

