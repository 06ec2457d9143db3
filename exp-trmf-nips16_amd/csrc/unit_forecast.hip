// unit_forecast.hip -- forecast_rollout_kernel and the explicit instantiations of forecast_score_kernel: the next timestamps of a
// resident model, forecast and scored on the device (kernel_units.hpp: one translation unit per kernel family, compiled in parallel).
#define TRMF_UNIT 6
#include "kernel_units.hpp"

namespace trmf {
TRMF_UNIT_FORECAST(TRMF_DEFINE_KERNEL)
}  // namespace trmf
