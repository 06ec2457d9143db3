// unit_slide.hip -- csc_slide_count_kernel, csc_slide_kernel and the explicit instantiations of series_downdate_kernel: the sliding
// window behind trmf_session_slide (kernel_units.hpp: one translation unit per kernel family).
#define TRMF_UNIT 14
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_SLIDE(TRMF_DEFINE_KERNEL)
}  // namespace trmf
