// unit_heldout.hip -- explicit instantiations of heldout_eval_kernel: the model at a resident set of held-out positions
// (kernel_units.hpp: one translation unit per kernel family, compiled in parallel).
#define TRMF_UNIT 5
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_HELDOUT(TRMF_DEFINE_KERNEL)
}  // namespace trmf
