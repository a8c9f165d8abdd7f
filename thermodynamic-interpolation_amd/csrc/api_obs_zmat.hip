// api_obs_zmat.hip -- C ABI of the Z-matrix coordinates both ways (include/ti_hip.h ti_obs_zmat, ti_obs_zmat_xyz): the topology
// checks and the staging.  Kernels: obs_zmat_kernels.hip.
#include "ti_handle.hpp"

// The checks ti_obs_zmat and ti_obs_zmat_xyz share, all before any device work; on TI_OK `topo` holds order [A] then ref [A][3].
static int zmat_check(ti_handle* h, const int32_t* order, const int32_t* ref, int mem, std::vector<int32_t>& topo)
{
    if (!h || h->kind != 0) return fail(TI_E_ARG, "not a painn handle");
    if (mem != TI_MEM_HOST && mem != TI_MEM_DEVICE) return fail(TI_E_ARG, "unknown mem");
    const int A = h->d.n_atoms;
    if (A < 2 || A > ZMAT_MAX_ATOMS) return fail(TI_E_ARG, "a Z-matrix needs 2 <= A <= " + std::to_string(ZMAT_MAX_ATOMS) + ", the handle has A = " + std::to_string(A));
    if (!h->natoms.empty()) return fail(TI_E_UNSUPPORTED, "one topology is one species: clear ti_painn_set_molecules first");
    if (!ref) return fail(TI_E_ARG, "ref is NULL");
    topo.assign((size_t)4 * A, 0);
    std::vector<char> seen((size_t)A, 0);
    for (int s = 0; s < A; ++s) {
        const int a = order ? order[s] : s;
        if (a < 0 || a >= A || seen[a]) return fail(TI_E_ARG, "order is not a permutation of 0.." + std::to_string(A - 1) + " (entry " + std::to_string(s) + ")");
        seen[a] = 1;
        topo[s] = a;
    }
    for (int s = 1; s < A; ++s) {
        const int n = s < 3 ? s : 3;                           // the slots that are read
        for (int j = 0; j < n; ++j) {
            const int r = ref[3 * s + j];
            if (r < 0 || r >= s) return fail(TI_E_ARG, "ref[" + std::to_string(s) + "][" + std::to_string(j) + "] = " + std::to_string(r) + " is not an earlier sorted atom");
            for (int j2 = 0; j2 < j; ++j2)
                if (ref[3 * s + j2] == r) return fail(TI_E_ARG, "ref[" + std::to_string(s) + "] repeats atom " + std::to_string(r));
            topo[A + 3 * s + j] = r;
        }
    }
    return TI_OK;
}

extern "C" {

int ti_obs_zmat(ti_handle* h, const int32_t* order, const int32_t* ref, const float* x, int64_t B, float* out_z, int mem)
{
    std::vector<int32_t> topo;
    if (int rc = zmat_check(h, order, ref, mem, topo)) return rc;
    if (B < 0 || (B > 0 && (!x || !out_z))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        const int A = h->d.n_atoms;
        h->zm_topo.upload(topo);
        Staged sg(h, mem);
        ZmatParams p{};
        p.x = sg.in(x, h->obs_x, (size_t)B * 3 * A);
        p.B = B; p.A = A; p.topo = h->zm_topo.p;
        p.z = sg.out(out_z, h->zm_z, (size_t)B * 3 * (A - 1));
        HIP_CHECK(launch_obs_zmat(p, h->stream));
        sg.finish();
        return TI_OK;
    });
}

int ti_obs_zmat_xyz(ti_handle* h, const int32_t* order, const int32_t* ref, const float* z, int64_t B, float* out_x, double* out_logdet,
                    uint8_t* out_valid, int mem)
{
    std::vector<int32_t> topo;
    if (int rc = zmat_check(h, order, ref, mem, topo)) return rc;
    if (B < 0 || (B > 0 && (!z || !out_x))) return fail(TI_E_ARG, "NULL buffer");
    if (B == 0) return TI_OK;
    return guarded([&]() -> int {
        set_device(h);
        const int A = h->d.n_atoms;
        h->zm_topo.upload(topo);
        Staged sg(h, mem);
        ZmatXyzParams p{};
        p.z = sg.in(z, h->zm_z, (size_t)B * 3 * (A - 1));
        p.B = B; p.A = A; p.topo = h->zm_topo.p;
        p.x = sg.out(out_x, h->obs_x, (size_t)B * 3 * A);
        p.logdet = out_logdet ? sg.out(out_logdet, h->zm_logdet, (size_t)B) : nullptr;
        p.valid = out_valid ? sg.out(out_valid, h->zm_valid, (size_t)B) : nullptr;
        HIP_CHECK(launch_obs_zmat_xyz(p, h->stream));
        sg.finish();
        return TI_OK;
    });
}

}  // extern "C"
