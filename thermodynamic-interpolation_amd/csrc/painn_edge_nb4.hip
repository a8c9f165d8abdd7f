// painn_edge_nb4.hip -- edge-kernel instantiations for n_features = 128 (painn_edge_kernel.hpp)
#include "painn_edge_kernel.hpp"

namespace ti {
template hipError_t configure_edge_unit<4, false>();
template hipError_t launch_edge_unit<4, false>(bool, bool, int, const EdgeParams&, hipStream_t);
}  // namespace ti
