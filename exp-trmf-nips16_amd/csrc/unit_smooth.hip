// unit_smooth.hip -- smooth_ar_kernel, smooth_apply_kernel, smooth_update_kernel, smooth_finish_kernel: the windowed preconditioned
// conjugate gradients behind trmf_session_smooth (kernel_units.hpp: one translation unit per kernel family).  None is a template:
// their bodies are compiled where TRMF_UNIT_BODIES is defined, i.e. here alone among the units.
#define TRMF_UNIT 11
#include "kernel_units.hpp"
