// painn_pair_mask_nb4.hip -- masked pair-major message kernel instantiations (per-molecule edge sets) for n_features = 128 (painn_pair_kernel.hpp)
#include "painn_pair_kernel.hpp"

namespace ti {
template hipError_t configure_pair_unit<4, true, false>();
template hipError_t launch_pair_unit<4, true, false>(bool, bool, int, const EdgeParams&, hipStream_t, bool);
}  // namespace ti
