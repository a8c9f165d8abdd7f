// painn_pair_tails_nb4.hip -- pair-major message kernel instantiations of the merged-tails general builds for n_features = 128 (painn_pair_kernel.hpp)
#include "painn_pair_kernel.hpp"

namespace ti {
template hipError_t configure_pair_tails_unit<4>();
template hipError_t launch_pair_tails_unit<4>(bool, bool, const EdgeParams&, hipStream_t, bool);
}  // namespace ti
