// OrientationState instantiations of the state-measurement kernel (fp64, fp32, fp32-wide)
#include "ukf_state_meas_launch.inc.hpp"

namespace ukfb {
int launch_state_meas_orient(ukfb_engine* e, const StateMeasReq& r) { return launch_state_meas_model<OrientM<double>, OrientM<float>>(e, r); }
}  // namespace ukfb
