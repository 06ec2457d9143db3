// unit_adapt.hip -- the kernels of the full-observation forms and the explicit instantiations of adapt_series_kernel / adapt_part_kernel:
// online loading updates behind trmf_session_adapt_series (kernel_units.hpp: one translation unit per kernel family).
#define TRMF_UNIT 10
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_ADAPT(TRMF_DEFINE_KERNEL)
}  // namespace trmf
