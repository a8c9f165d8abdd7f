// painn_pair_seed_nb4.hip -- pair-major message kernel instantiations of the seeded builds, tile and general, for n_features = 128 (painn_pair_kernel.hpp)
#include "painn_pair_kernel.hpp"

namespace ti {
template hipError_t configure_pair_unit<4, false, false, true>();
template hipError_t launch_pair_unit<4, false, false, true>(bool, bool, int, const EdgeParams&, hipStream_t, bool);
template hipError_t configure_pair_unit<4, false, true, true>();
template hipError_t launch_pair_unit<4, false, true, true>(bool, bool, int, const EdgeParams&, hipStream_t, bool);
}  // namespace ti
