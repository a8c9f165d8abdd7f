// painn_pair_nb4.hip -- pair-major message kernel instantiations for n_features = 128 (painn_pair_kernel.hpp)
#include "painn_pair_kernel.hpp"

namespace ti {
template hipError_t configure_pair_unit<4, false, false>();
template hipError_t launch_pair_unit<4, false, false>(bool, bool, int, const EdgeParams&, hipStream_t, bool);
}  // namespace ti
