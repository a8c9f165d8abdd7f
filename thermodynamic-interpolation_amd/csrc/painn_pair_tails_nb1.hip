// painn_pair_tails_nb1.hip -- pair-major message kernel instantiations of the merged-tails general builds for n_features = 32 (painn_pair_kernel.hpp)
#include "painn_pair_kernel.hpp"

namespace ti {
template hipError_t configure_pair_tails_unit<1>();
template hipError_t launch_pair_tails_unit<1>(bool, bool, const EdgeParams&, hipStream_t, bool);
}  // namespace ti
