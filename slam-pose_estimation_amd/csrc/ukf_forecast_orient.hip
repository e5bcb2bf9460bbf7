// OrientationState instantiations of the forecast kernel (fp64, fp32, fp32-wide)
#include "ukf_forecast_launch.inc.hpp"

namespace ukfb {
int launch_forecast_orient(ukfb_engine* e, const ForecastReq& r) { return launch_forecast_model<OrientM<double>, OrientM<float>>(e, r); }
}  // namespace ukfb
