// painn_pair_mask_nb2.hip -- masked pair-major message kernel instantiations (per-molecule edge sets) for n_features = 64 (painn_pair_kernel.hpp)
#include "painn_pair_kernel.hpp"

namespace ti {
hipError_t configure_pair_mask_nb2() { return configure_pair_nb<2, true>(); }
hipError_t launch_pair_mask_nb2(bool first, bool last, int prec, const EdgeParams& p, hipStream_t st) { return launch_pair_nb<2, true>(first, last, prec, p, st); }
}  // namespace ti
