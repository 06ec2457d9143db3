// unit_uncertainty.hip -- the noise fit (noise_resid_kernel and its reductions, noise_innov_kernel), forecast_psi_kernel and the
// explicit instantiations of forecast_dist_kernel: the predictive distribution of a forecast (kernel_units.hpp: one translation
// unit per kernel family, compiled in parallel).
#define TRMF_UNIT 8
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_UNCERTAINTY(TRMF_DEFINE_KERNEL)
}  // namespace trmf
