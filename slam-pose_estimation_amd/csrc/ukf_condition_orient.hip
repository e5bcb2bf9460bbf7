// OrientationState instantiations of the conditioning kernel (fp64, fp32, fp32-wide)
#include "ukf_condition_launch.inc.hpp"

namespace ukfb {
int launch_condition_orient(ukfb_engine* e, const ConditionReq& r) { return launch_condition_model<OrientM<double>, OrientM<float>>(e, r); }
}  // namespace ukfb
