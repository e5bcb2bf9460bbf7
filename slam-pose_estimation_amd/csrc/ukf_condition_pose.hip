// PoseWithVelocity instantiations of the conditioning kernel (fp64, fp32, fp32-wide)
#include "ukf_condition_launch.inc.hpp"

namespace ukfb {
int launch_condition_pose(ukfb_engine* e, const ConditionReq& r) { return launch_condition_model<PoseM<double>, PoseM<float>>(e, r); }
}  // namespace ukfb
