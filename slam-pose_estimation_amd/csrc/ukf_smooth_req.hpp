// ukf_smooth_req.hpp -- untyped request of one smoother launch; the typed SmoothArgs<T, TS> is built inside the per-model
// translation units (ukf_smooth_pose.hip, ukf_smooth_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

struct SmoothReq {
    int slots = 1;
    SmoothLaunch part{};                  // which backward steps (SmoothPlan, ukf_host.hpp)
    const double* dt = nullptr;           // HOST [steps - 1], the whole window's
    const void* mu_hist_dev = nullptr;    // [slots][capacity][S]
    const void* cov_hist_dev = nullptr;   // [slots][capacity][PK]
    const void* in_a_dev = nullptr;       // [slots][capacity][3] or null (the engine's latched inputs)
    const void* in_b_dev = nullptr;
    void* mu_out_dev = nullptr;
    void* cov_out_dev = nullptr;          // may be null
    const void* start_cov_dev = nullptr;  // [capacity][PK]: the chain's covariance at part.top_step
    void* end_cov_dev = nullptr;          // [capacity][PK] or null
    uint32_t* status_dev = nullptr;       // [capacity] or null
};

int launch_smooth_pose(ukfb_engine* e, const SmoothReq& r);
int launch_smooth_orient(ukfb_engine* e, const SmoothReq& r);

}  // namespace ukfb
