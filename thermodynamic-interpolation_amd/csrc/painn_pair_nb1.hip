// painn_pair_nb1.hip -- pair-major message kernel instantiations for n_features = 32 (painn_pair_kernel.hpp)
#include "painn_pair_kernel.hpp"

namespace ti {
template hipError_t configure_pair_unit<1, false, false>();
template hipError_t launch_pair_unit<1, false, false>(bool, bool, int, const EdgeParams&, hipStream_t, bool);
}  // namespace ti
