// ukf_delayed_req.hpp -- untyped request of one delayed-measurement launch; the typed DelayedArgs<T, TS> is built inside the
// per-model translation units (ukf_delayed_pose.hip, ukf_delayed_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct DelayedReq {
    ukfb_delayed_in in{};     // in.dt: HOST [steps - 1], copied into the kernel arguments
    bool commit = false;
    ukfb_delayed_out out{};   // all NULL when the caller passed none
};

int launch_delayed_pose(ukfb_engine* e, const DelayedReq& r);
int launch_delayed_orient(ukfb_engine* e, const DelayedReq& r);

}  // namespace ukfb
