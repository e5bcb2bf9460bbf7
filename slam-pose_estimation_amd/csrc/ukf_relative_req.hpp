// ukf_relative_req.hpp -- untyped request of one relative-measurement launch; the typed RelativeArgs<T, TS> is built inside the
// per-model translation unit (ukf_relative_pose.hip: the feature serves Pose engines only).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct RelativeReq {
    ukfb_relative_in in{};     // in.dt: HOST [steps - 1], copied into the kernel arguments
    bool commit = false;
    ukfb_relative_out out{};   // all NULL when the caller passed none
};

int launch_relative_pose(ukfb_engine* e, const RelativeReq& r);

}  // namespace ukfb
