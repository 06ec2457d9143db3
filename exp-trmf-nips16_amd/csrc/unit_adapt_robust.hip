// unit_adapt_robust.hip -- the objective kernel and the explicit instantiations of adapt_robust_series_kernel: robust online loading
// updates behind trmf_session_adapt_series_robust (kernel_units.hpp: one translation unit per kernel family).
#define TRMF_UNIT 13
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_ADAPT_ROBUST(TRMF_DEFINE_KERNEL)
}  // namespace trmf
