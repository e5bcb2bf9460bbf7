// PoseWithVelocity instantiations of the smoother kernel (fp64, fp32, fp32-wide)
#include "ukf_smooth_launch.inc.hpp"

namespace ukfb {
int launch_smooth_pose(ukfb_engine* e, const SmoothReq& r) { return launch_smooth_model<PoseM<double>, PoseM<float>>(e, r); }
}  // namespace ukfb
