// ukf_forecast_req.hpp -- untyped request of the forecast launch; the typed ForecastArgs<T, TS> is built inside the per-model
// translation units (ukf_forecast_pose.hip, ukf_forecast_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct ForecastReq {
    int steps = 1, slots = 1, first_slot = 0;
    const double* dt = nullptr;            // HOST [steps], or null
    const int64_t* ts_us = nullptr;        // HOST [steps], or null: exactly one of the two
    const void* start_mu_dev = nullptr;    // [capacity][S], or null (with start_cov_dev): the engine's state
    const void* start_cov_dev = nullptr;   // [capacity][PK]
    const void* in_a_dev = nullptr;        // [slots][capacity][3] or null (the engine's latched inputs)
    const void* in_b_dev = nullptr;
    void* mu_out_dev = nullptr;            // [slots][capacity][S]
    void* cov_out_dev = nullptr;           // [slots][capacity][PK], may be null
    uint32_t* status_dev = nullptr;        // [capacity] or null
};

int launch_forecast_pose(ukfb_engine* e, const ForecastReq& r);
int launch_forecast_orient(ukfb_engine* e, const ForecastReq& r);

}  // namespace ukfb
