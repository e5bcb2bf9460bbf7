// PoseWithVelocity instantiations of the innovation kernel (fp64, fp32, fp32-wide)
#include "ukf_innovation_launch.inc.hpp"

namespace ukfb {
int launch_innovation_pose(ukfb_engine* e, const InnovReq& r) { return launch_innovation_model<PoseM<double>, PoseM<float>>(e, r); }
}  // namespace ukfb
