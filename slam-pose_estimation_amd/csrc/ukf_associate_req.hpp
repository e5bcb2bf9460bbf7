// ukf_associate_req.hpp -- untyped request of one sensor-frame association launch; the typed AssociateArgs<T, TS> is built
// inside the per-model translation units (ukf_associate_pose.hip, ukf_associate_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct AssociateReq {
    int model_uniform = -1;
    ukfb_associate_in in{};    // device pointers and the by-value mount / point
    bool commit = false;
    ukfb_associate_out out{};  // any may be null
};

int launch_associate_pose(ukfb_engine* e, const AssociateReq& r);
int launch_associate_orient(ukfb_engine* e, const AssociateReq& r);

}  // namespace ukfb
