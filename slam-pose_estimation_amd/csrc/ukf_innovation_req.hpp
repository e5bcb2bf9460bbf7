// ukf_innovation_req.hpp -- untyped request of the innovation / candidate-selection launches; the typed InnovArgs<T> is built
// inside the per-model translation units (ukf_innovation_pose.hip, ukf_innovation_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct InnovReq {
    int meas_uniform = -1;
    const int32_t* meas_dev = nullptr;
    int candidates = 1;
    const void* z_dev = nullptr;
    const void* Q_dev = nullptr;
    bool q_uniform = false;
    ukfb_innovation_out out{};
};

int launch_innovation_pose(ukfb_engine* e, const InnovReq& r);
int launch_innovation_orient(ukfb_engine* e, const InnovReq& r);

}  // namespace ukfb
