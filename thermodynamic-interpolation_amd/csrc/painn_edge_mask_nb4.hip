// painn_edge_mask_nb4.hip -- masked edge-kernel instantiations (per-molecule edge sets) for n_features = 128 (painn_edge_kernel.hpp)
#include "painn_edge_kernel.hpp"

namespace ti {
template hipError_t configure_edge_unit<4, true>();
template hipError_t launch_edge_unit<4, true>(bool, bool, int, const EdgeParams&, hipStream_t);
}  // namespace ti
