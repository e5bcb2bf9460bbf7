// ukf_sensor_meas_req.hpp -- untyped request of one sensor-frame measurement launch; the typed SensorArgs<T, TS> is built inside
// the per-model translation units (ukf_sensor_meas_pose.hip, ukf_sensor_meas_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct SensorReq {
    int model_uniform = -1;
    ukfb_sensor_in in{};      // device pointers and the by-value mount / point
    bool commit = false;
    ukfb_sensor_out out{};    // any may be null
};

int launch_sensor_meas_pose(ukfb_engine* e, const SensorReq& r);
int launch_sensor_meas_orient(ukfb_engine* e, const SensorReq& r);

}  // namespace ukfb
