// painn_edge_mask_nb8.hip -- masked edge-kernel instantiations (per-molecule edge sets) for n_features = 256 (painn_edge_kernel.hpp)
#include "painn_edge_kernel.hpp"

namespace ti {
hipError_t configure_edge_mask_nb8() { return configure_edge_nb<8, true>(); }
hipError_t launch_edge_mask_nb8(bool first, bool last, int prec, const EdgeParams& p, hipStream_t st) { return launch_edge_nb<8, true>(first, last, prec, p, st); }
}  // namespace ti
