// PoseWithVelocity instantiations of the filter-bank kernels (fp64, fp32, fp32-wide), and the model-independent weights kernel
#include "ukf_bank_launch.inc.hpp"

namespace ukfb {
int launch_bank_pose(ukfb_engine* e, const BankReq& r) { return launch_bank_model<PoseM<double>, PoseM<float>>(e, r); }
int launch_bank_weights(ukfb_engine* e, const BankWeightsReq& r) {
    if (e->prec == UKFB_F64) return launch_bank_weights_typed<double, double>(e, r);
    if (e->cfg.wide_arithmetic) return launch_bank_weights_typed<float, double>(e, r);
    return launch_bank_weights_typed<float, float>(e, r);
}
}  // namespace ukfb
