// PoseWithVelocity instantiations of the sigma-point export and the sampled-update kernel (fp64, fp32, fp32-wide)
#include "ukf_sampled_launch.inc.hpp"

namespace ukfb {
int launch_sigma_points_pose(ukfb_engine* e, const SigmaPointsReq& r) { return launch_sigma_points_model<PoseM<double>, PoseM<float>>(e, r); }
int launch_sampled_pose(ukfb_engine* e, const SampledReq& r) { return launch_sampled_model<PoseM<double>, PoseM<float>>(e, r); }
}  // namespace ukfb
