// painn_update_keep.hip -- the update kernel's builds that keep v_eff in registers between their phases instead of parking it in
// dvacc (painn_update_kernel_body.inc: KEEP): the twins of the f16x2 builds of painn_kernels.hip up to F = 128.
// A unit of its own, so that the code objects of painn_kernels.hip stay as they were and remain in the library for TI_UPDATE_KEEP=0.
#include "dispatch.hpp"
#include "mfma_chain.hpp"
#include "painn_update_kernel.hpp"
#include "ti_internal.hpp"

namespace ti {

// update_keep: the components kept, per width -- the most at which the build has no scratch, still runs two workgroups per CU and
// gives the bits of the parked builds (profiles/update_keep_resources.txt).  At F = 128 a third row does not fit (22 - 32 registers
// too many); at F = 32 and 64 it fits, but those builds moved s and v by an ulp (profiles/update_keep_bench.txt) and are not shipped.
__host__ __device__ constexpr int update_keep(int NBK) { return NBK <= 8 ? 2 : 0; }
constexpr bool update_keep_build_exists(int nb, int prec) { return prec == TI_PREC_F16X2 && nb <= 4; }

#define TI_UPDATE_KEEP update_keep(NBK)
template <int NBK, bool HAS_NEXT, bool FOLDED, int PREC = 1>
__global__ __launch_bounds__(256, 2) void painn_update_keep_kernel(const UpdateParams p)
#define TI_UPDATE_SCLS false
#include "painn_update_kernel_body.inc"
#undef TI_UPDATE_SCLS

// layer 0's update after an embed per class (painn_update_cls_kernel's twin)
template <int NBK, bool HAS_NEXT, bool FOLDED = false, int PREC = 1>
__global__ __launch_bounds__(256, 2) void painn_update_cls_keep_kernel(const UpdateParams p)
#define TI_UPDATE_SCLS true
#include "painn_update_kernel_body.inc"
#undef TI_UPDATE_SCLS
#undef TI_UPDATE_KEEP

// f(kernel) for every build that (NB, has_next, folded, per class) select (EVERY: all of them), until one returns an error; the
// per-class builds exist where the layer-0 phi table does and are never folded, as their twins (painn_kernels.hip: node_build_exists)
template <class F>
static hipError_t with_keep_builds(int NB, int has_next, int folded, int cls, F&& f)
{
    hipError_t e = hipSuccess;
    bool any = false;
    dispatch_int<1, 2, 4>(NB, [&](auto bc) { dispatch_bool(has_next, [&](auto hc) { dispatch_bool(folded, [&](auto fc) { dispatch_bool(cls, [&](auto cc) {
        constexpr int nb = decltype(bc)::value;
        constexpr bool HAS_NEXT = decltype(hc)::value, FOLDED = decltype(fc)::value, CLS = decltype(cc)::value;
        if constexpr (!CLS) {
            any = true;
            if (e == hipSuccess) e = f(painn_update_keep_kernel<2 * nb, HAS_NEXT, FOLDED>);
        } else if constexpr (!FOLDED && pair_table_build_exists(nb, TI_PREC_F16X2, false)) {
            any = true;
            if (e == hipSuccess) e = f(painn_update_cls_keep_kernel<2 * nb, HAS_NEXT>);
        }
    }); }); }); });
    return any ? e : hipErrorInvalidValue;
}

int update_keep_components(int NB, int prec) { return update_keep_build_exists(NB, prec) ? update_keep(2 * NB) : 0; }

hipError_t configure_update_keep(int NB)
{
    if (!update_keep_build_exists(NB, TI_PREC_F16X2)) return hipSuccess;
    return with_keep_builds(NB, EVERY, EVERY, EVERY, [&](auto kernel) { return set_lds(kernel, update_lds_bytes(NB, false)); });
}

hipError_t launch_update_keep(int NB, bool has_next, int prec, const UpdateParams& p, hipStream_t st, bool folded)
{
    if (!update_keep_build_exists(NB, prec)) return hipErrorInvalidValue;
    return with_keep_builds(NB, has_next, folded, p.s_cls != nullptr, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((p.N + 63) / 64)), dim3(256), update_lds_bytes(NB, false), st, p);       // 4 waves x 16 atoms per workgroup
        return hipGetLastError();
    });
}

}  // namespace ti
