// PoseWithVelocity instantiations of the relative-measurement kernel (fp64, fp32, fp32-wide); the feature has no other model
#include "ukf_relative_launch.inc.hpp"

namespace ukfb {
int launch_relative_pose(ukfb_engine* e, const RelativeReq& r) { return launch_relative_model<PoseM<double>, PoseM<float>>(e, r); }
}  // namespace ukfb
