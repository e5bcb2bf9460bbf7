// ukf_condition_req.hpp -- untyped request of one conditioning launch; the typed ConditionArgs<T, TS> is built inside the
// per-model translation units (ukf_condition_pose.hip, ukf_condition_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct ConditionReq {
    ukfb_condition_in in{};     // device pointers
    bool commit = false;
    ukfb_condition_out out{};   // any may be null
};

int launch_condition_pose(ukfb_engine* e, const ConditionReq& r);
int launch_condition_orient(ukfb_engine* e, const ConditionReq& r);

}  // namespace ukfb
