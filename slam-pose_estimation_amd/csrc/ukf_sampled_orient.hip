// OrientationState instantiations of the sigma-point export and the sampled-update kernel (fp64, fp32, fp32-wide)
#include "ukf_sampled_launch.inc.hpp"

namespace ukfb {
int launch_sigma_points_orient(ukfb_engine* e, const SigmaPointsReq& r) { return launch_sigma_points_model<OrientM<double>, OrientM<float>>(e, r); }
int launch_sampled_orient(ukfb_engine* e, const SampledReq& r) { return launch_sampled_model<OrientM<double>, OrientM<float>>(e, r); }
}  // namespace ukfb
