// ukf_sampled_req.hpp -- untyped requests of the sigma-point export and of one sampled-update launch; the typed SigmaPointsArgs /
// SampledArgs<T, TS> are built inside the per-model translation units (ukf_sampled_pose.hip, ukf_sampled_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct SigmaPointsReq {
    void* X = nullptr;            // either may be null, not both
    void* delta = nullptr;
    uint32_t* status = nullptr;   // may be null
};

struct SampledReq {
    ukfb_sampled_in in{};     // device pointers
    bool commit = false;
    ukfb_sampled_out out{};   // any may be null
};

int launch_sigma_points_pose(ukfb_engine* e, const SigmaPointsReq& r);
int launch_sigma_points_orient(ukfb_engine* e, const SigmaPointsReq& r);
int launch_sampled_pose(ukfb_engine* e, const SampledReq& r);
int launch_sampled_orient(ukfb_engine* e, const SampledReq& r);

}  // namespace ukfb
