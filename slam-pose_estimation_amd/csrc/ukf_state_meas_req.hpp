// ukf_state_meas_req.hpp -- untyped request of one state-measurement launch; the typed StateMeasArgs<T, TS> is built inside the
// per-model translation units (ukf_state_meas_pose.hip, ukf_state_meas_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct StateMeasReq {
    uint32_t mask_uniform = 0;
    const int32_t* mask_dev = nullptr;   // [capacity] or null
    const void* z_dev = nullptr;         // [capacity][S]
    const void* Qz_dev = nullptr;        // [capacity][PK]
    double state_inflation = 1.0, meas_inflation = 1.0;
    bool commit = false;
    ukfb_state_meas_out out{};           // any may be null
};

int launch_state_meas_pose(ukfb_engine* e, const StateMeasReq& r);
int launch_state_meas_orient(ukfb_engine* e, const StateMeasReq& r);

}  // namespace ukfb
