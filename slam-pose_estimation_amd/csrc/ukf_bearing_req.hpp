// ukf_bearing_req.hpp -- untyped request of one bearing measurement launch; the typed SensorArgs<T, TS> is built inside
// the per-model translation units (ukf_bearing_pose.hip, ukf_bearing_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct BearingReq {
    int model_uniform = -1;
    ukfb_sensor_in in{};      // device pointers and the by-value mount / point
    bool commit = false;
    ukfb_sensor_out out{};    // any may be null
};

int launch_bearing_pose(ukfb_engine* e, const BearingReq& r);
int launch_bearing_orient(ukfb_engine* e, const BearingReq& r);

}  // namespace ukfb
