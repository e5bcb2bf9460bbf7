// OrientationState instantiations of the sampled-prediction kernel (fp64, fp32, fp32-wide)
#include "ukf_predict_sampled_launch.inc.hpp"

namespace ukfb {
int launch_predict_sampled_orient(ukfb_engine* e, const PredictSampledReq& r) { return launch_predict_sampled_model<OrientM<double>, OrientM<float>>(e, r); }
}  // namespace ukfb
