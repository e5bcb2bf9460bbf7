// ukf_predict_sampled_req.hpp -- untyped request of one sampled-prediction launch; the typed PredictSampledArgs<T, TS> is built
// inside the per-model translation units (ukf_predict_sampled_pose.hip, ukf_predict_sampled_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct PredictSampledReq {
    ukfb_predict_sampled_in in{};     // device pointers
    bool commit = false;
    ukfb_predict_sampled_out out{};   // any may be null
};

int launch_predict_sampled_pose(ukfb_engine* e, const PredictSampledReq& r);
int launch_predict_sampled_orient(ukfb_engine* e, const PredictSampledReq& r);

}  // namespace ukfb
