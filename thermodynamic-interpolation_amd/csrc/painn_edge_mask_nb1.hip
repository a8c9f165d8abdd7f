// painn_edge_mask_nb1.hip -- masked edge-kernel instantiations (per-molecule edge sets) for n_features = 32 (painn_edge_kernel.hpp)
#include "painn_edge_kernel.hpp"

namespace ti {
hipError_t configure_edge_mask_nb1() { return configure_edge_nb<1, true>(); }
hipError_t launch_edge_mask_nb1(bool first, bool last, int prec, const EdgeParams& p, hipStream_t st) { return launch_edge_nb<1, true>(first, last, prec, p, st); }
}  // namespace ti
