// ukf_bank_req.hpp -- untyped requests of the filter-bank launches; the typed BankArgs<T, TS> are built inside the per-model
// translation units (ukf_bank_pose.hip, ukf_bank_orient.hip).
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

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

int launch_bank_pose(ukfb_engine* e, const BankReq& r);
int launch_bank_orient(ukfb_engine* e, const BankReq& r);
int launch_bank_weights(ukfb_engine* e, const BankWeightsReq& r);   // model-independent (ukf_bank_pose.hip)

}  // namespace ukfb
