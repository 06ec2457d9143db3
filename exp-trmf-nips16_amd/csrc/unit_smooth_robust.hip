// unit_smooth_robust.hip -- the explicit instantiations of smooth_robust_part_kernel / smooth_robust_fold_kernel: the weighted Grams of
// the robust smoother behind trmf_session_smooth_robust (kernel_units.hpp: one translation unit per kernel family).
#define TRMF_UNIT 12
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_SMOOTH_ROBUST(TRMF_DEFINE_KERNEL)
}  // namespace trmf
