// OrientationState instantiations of the filter-bank kernels (fp64, fp32, fp32-wide)
#include "ukf_bank_launch.inc.hpp"

namespace ukfb {
int launch_bank_orient(ukfb_engine* e, const BankReq& r) { return launch_bank_model<OrientM<double>, OrientM<float>>(e, r); }
}  // namespace ukfb
