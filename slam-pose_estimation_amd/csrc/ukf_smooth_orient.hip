// OrientationState instantiations of the smoother kernel (fp64, fp32, fp32-wide)
#include "ukf_smooth_launch.inc.hpp"

namespace ukfb {
int launch_smooth_orient(ukfb_engine* e, const SmoothReq& r) { return launch_smooth_model<OrientM<double>, OrientM<float>>(e, r); }
}  // namespace ukfb
