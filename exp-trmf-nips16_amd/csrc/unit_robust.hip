// unit_robust.hip -- assim_robust_prior_kernel and the explicit instantiations of assim_robust_part_kernel / assim_robust_solve_kernel:
// the Huber-weighted forward filter behind trmf_session_assimilate_robust (kernel_units.hpp: one translation unit per kernel family).
#define TRMF_UNIT 9
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_ROBUST(TRMF_DEFINE_KERNEL)
}  // namespace trmf
