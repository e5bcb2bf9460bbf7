// PoseWithVelocity instantiations of the sampled-prediction kernel (fp64, fp32, fp32-wide)
#include "ukf_predict_sampled_launch.inc.hpp"

namespace ukfb {
int launch_predict_sampled_pose(ukfb_engine* e, const PredictSampledReq& r) { return launch_predict_sampled_model<PoseM<double>, PoseM<float>>(e, r); }
}  // namespace ukfb
