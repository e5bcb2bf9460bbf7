// OrientationState instantiations of the sensor-frame association kernel (fp64, fp32, fp32-wide; shared-h and per-hypothesis)
#include "ukf_associate_launch.inc.hpp"

namespace ukfb {
int launch_associate_orient(ukfb_engine* e, const AssociateReq& r) { return launch_associate_model<OrientM<double>, OrientM<float>>(e, r); }
}  // namespace ukfb
