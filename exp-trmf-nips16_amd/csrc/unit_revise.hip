// unit_revise.hip -- revise_count_kernel, revise_kernel, dense_revise_kernel and series_revise_kernel (4): cell revisions behind
// trmf_session_revise (kernel_units.hpp: one translation unit per kernel family).
#define TRMF_UNIT 16
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_REVISE(TRMF_DEFINE_KERNEL)
}  // namespace trmf
