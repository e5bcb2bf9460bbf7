// OrientationState instantiations of the delayed-measurement kernel (fp64, fp32, fp32-wide)
#include "ukf_delayed_launch.inc.hpp"

namespace ukfb {
int launch_delayed_orient(ukfb_engine* e, const DelayedReq& r) { return launch_delayed_model<OrientM<double>, OrientM<float>>(e, r); }
}  // namespace ukfb
