// PoseWithVelocity instantiations of the bearing measurement kernel (fp64, fp32, fp32-wide)
#include "ukf_bearing_launch.inc.hpp"

namespace ukfb {
int launch_bearing_pose(ukfb_engine* e, const BearingReq& r) { return launch_bearing_model<PoseM<double>, PoseM<float>>(e, r); }
}  // namespace ukfb
