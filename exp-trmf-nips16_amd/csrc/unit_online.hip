// unit_online.hip -- assim_chain_kernel, assim_err_kernel and the explicit instantiations of assim_factor_kernel: the forward filter
// behind trmf_session_assimilate (kernel_units.hpp: one translation unit per kernel family, compiled in parallel).
#define TRMF_UNIT 7
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_ONLINE(TRMF_DEFINE_KERNEL)
}  // namespace trmf
