// painn_edge_mask_nb1.hip -- masked edge-kernel instantiations (per-molecule edge sets) for n_features = 32 (painn_edge_kernel.hpp)
#include "painn_edge_kernel.hpp"

namespace ti {
template hipError_t configure_edge_unit<1, true>();
template hipError_t launch_edge_unit<1, true>(bool, bool, int, const EdgeParams&, hipStream_t);
}  // namespace ti
