// ukf_feature_req.hpp -- the untyped requests that the C ABI of the features (ukf_<feature>_api.hip) hands to
// launch_for_model (ukf_feature_bind.hpp); the typed argument struct of a kernel is built inside the feature's
// ukf_<feature>_launch.hip.  Pointers named *_dev are device pointers; HOST arrays are copied into the kernel arguments.
#pragma once

#include "ukf_feature_bind.hpp"

namespace ukfb {

struct InnovReq {
    int meas_uniform = -1;
    const int32_t* meas_dev = nullptr;
    int candidates = 1;
    const void* z_dev = nullptr;
    const void* Q_dev = nullptr;
    bool q_uniform = false;
    ukfb_innovation_out out{};
};

struct BankReq {
    int hypotheses = 2;
    bool mix = false;                    // false: combine
    const void* w_dev = nullptr;         // [capacity]
    void* mu_out_dev = nullptr;          // combine: [tracks][S]
    void* cov_out_dev = nullptr;         // combine: [tracks][PK] or null
    void* w_pred_dev = nullptr;          // mix: [capacity]
    const double* transition = nullptr;  // mix: HOST [M][M], already checked
    uint32_t* status_dev = nullptr;      // [tracks] or null
};

struct BankWeightsReq {
    int hypotheses = 2;
    const void* logw_in_dev = nullptr;
    const void* loglik_dev = nullptr;
    void* logw_out_dev = nullptr;
    void* w_out_dev = nullptr;
    uint32_t* status_dev = nullptr;
};

int launch_bank_weights(ukfb_engine* e, const BankWeightsReq& r);   // model-independent (the Pose object of ukf_bank_launch.hip)

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

struct StateMeasReq {
    uint32_t mask_uniform = 0;
    const int32_t* mask_dev = nullptr;   // [capacity] or null
    const void* z_dev = nullptr;         // [capacity][S]
    const void* Qz_dev = nullptr;        // [capacity][PK]
    double state_inflation = 1.0, meas_inflation = 1.0;
    bool commit = false;
    ukfb_state_meas_out out{};           // any may be null
};

// One sensor-frame measurement launch; BEARING names the kernel: ukf_bearing_kernel, else ukf_sensor_meas_kernel
template <bool BEARING> struct SensorFrameReq {
    int model_uniform = -1;
    ukfb_sensor_in in{};      // device pointers and the by-value mount / point
    bool commit = false;
    ukfb_sensor_out out{};    // any may be null
};
using SensorReq = SensorFrameReq<false>;
using BearingReq = SensorFrameReq<true>;

struct AssociateReq {
    int model_uniform = -1;
    ukfb_associate_in in{};    // device pointers and the by-value mount / point
    bool commit = false;
    ukfb_associate_out out{};  // any may be null
};

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

struct PredictSampledReq {
    ukfb_predict_sampled_in in{};     // device pointers
    bool commit = false;
    ukfb_predict_sampled_out out{};   // any may be null
};

struct DelayedReq {
    ukfb_delayed_in in{};     // in.dt: HOST [steps - 1], copied into the kernel arguments
    bool commit = false;
    ukfb_delayed_out out{};   // all NULL when the caller passed none
};

struct ConditionReq {
    ukfb_condition_in in{};     // device pointers
    bool commit = false;
    ukfb_condition_out out{};   // any may be null
};

struct RelativeReq {
    ukfb_relative_in in{};     // in.dt: HOST [steps - 1], copied into the kernel arguments
    bool commit = false;
    ukfb_relative_out out{};   // all NULL when the caller passed none
};
template <> inline constexpr bool pose_only<RelativeReq> = true;

struct RobustReq {
    int model_uniform = -1;
    ukfb_sensor_in in{};      // device pointers and the by-value mount / point
    ukfb_robust_rule rule{};  // HOST values, already checked
    bool commit = false;
    ukfb_robust_out out{};    // any may be null
};

struct PdaReq {
    int model_uniform = -1;
    ukfb_associate_in in{};    // device pointers and the by-value mount / point; shared-h mode
    ukfb_pda_rule rule{};      // HOST values, already checked
    bool commit = false;
    ukfb_pda_out out{};        // any may be null
};

struct WeightedReq {
    int model_uniform = -1;
    ukfb_associate_in in{};    // device pointers and the by-value mount / point; shared-h mode
    const void* weight = nullptr;   // [candidates][capacity], engine precision
    bool commit = false;
    ukfb_weighted_out out{};   // any may be null
};

struct DelayedSensorReq {
    ukfb_delayed_sensor_in in{};   // in.dt: HOST [steps - 1], copied into the kernel arguments; the by-value mount / point
    bool commit = false;
    ukfb_delayed_out out{};        // all NULL when the caller passed none
};

}  // namespace ukfb
