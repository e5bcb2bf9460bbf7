// ukf_bank_api.hip -- C-ABI of the filter banks (include/ukf_batch.h, "filter banks"): argument checks (ukf_host.hpp), the
// launch requests, and the host-array forms.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

namespace {

int entry(ukfb_engine* e, int hypotheses) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (const int rc = ukfb::fail(ukfb::check_bank_args(hypotheses, e->cap))) return rc;
    return ukfb::refuse_poisoned(e);
}

}  // namespace

extern "C" {

int ukfb_bank_weights_dev(ukfb_engine* e, int hypotheses, const void* logw_in_dev, const void* loglik_dev, void* logw_out_dev,
                          void* w_out_dev, uint32_t* status_dev) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!logw_out_dev) return ukfb::fail({UKFB_ERR_INVALID_ARG, "logw_out must not be NULL"});
    ON_DEVICE(e->device);
    ukfb::BankWeightsReq r;
    r.hypotheses = hypotheses;
    r.logw_in_dev = logw_in_dev;
    r.loglik_dev = loglik_dev;
    r.logw_out_dev = logw_out_dev;
    r.w_out_dev = w_out_dev;
    r.status_dev = status_dev;
    return ukfb::launch_bank_weights(e, r);
}

int ukfb_bank_combine_dev(ukfb_engine* e, int hypotheses, const void* w_dev, void* mu_out_dev, void* cov_packed_out_dev,
                          uint32_t* status_dev) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!w_dev || !mu_out_dev) return ukfb::fail({UKFB_ERR_INVALID_ARG, "w and mu_out must not be NULL"});
    ON_DEVICE(e->device);
    ukfb::BankReq r;
    r.hypotheses = hypotheses;
    r.w_dev = w_dev;
    r.mu_out_dev = mu_out_dev;
    r.cov_out_dev = cov_packed_out_dev;
    r.status_dev = status_dev;
    return ukfb::launch_for_model(e, r);
}

int ukfb_bank_mix_dev(ukfb_engine* e, int hypotheses, const void* w_dev, const double* transition, void* w_pred_out_dev,
                      uint32_t* status_dev) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!w_dev || !w_pred_out_dev) return ukfb::fail({UKFB_ERR_INVALID_ARG, "w and w_pred_out must not be NULL"});
    if (const int rc = ukfb::fail(ukfb::check_bank_transition(transition, hypotheses))) return rc;
    ON_DEVICE(e->device);
    ukfb::BankReq r;
    r.hypotheses = hypotheses;
    r.mix = true;
    r.w_dev = w_dev;
    r.w_pred_dev = w_pred_out_dev;
    r.transition = transition;   // copied into the kernel arguments: nothing of the caller's is read after the call returns
    r.status_dev = status_dev;
    return ukfb::launch_for_model(e, r);
}

int ukfb_bank_combine(ukfb_engine* e, int hypotheses, const double* w, double* mu, double* cov, uint32_t* status) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!w || !mu) return ukfb::fail({UKFB_ERR_INVALID_ARG, "w and mu must not be NULL"});
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), tracks = n / size_t(hypotheses);
    ukfb::HostStage stage(e);
    const void* w_d = stage.in(w, n);
    void* mu_d = stage.out(mu, tracks * size_t(e->S));
    void* cov_d = stage.cov_out(cov, tracks);
    uint32_t* st_d = stage.raw_out(status, tracks);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_bank_combine_dev(e, hypotheses, w_d, mu_d, cov_d, st_d)) return rc;
    return stage.finish();
}

int ukfb_bank_mix(ukfb_engine* e, int hypotheses, const double* w, const double* transition, double* w_pred, uint32_t* status) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!w || !w_pred) return ukfb::fail({UKFB_ERR_INVALID_ARG, "w and w_pred must not be NULL"});
    if (const int rc = ukfb::fail(ukfb::check_bank_transition(transition, hypotheses))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), tracks = n / size_t(hypotheses);
    ukfb::HostStage stage(e);
    const void* w_d = stage.in(w, n);
    void* wp_d = stage.out(w_pred, n);
    uint32_t* st_d = stage.raw_out(status, tracks);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_bank_mix_dev(e, hypotheses, w_d, transition, wp_d, st_d)) return rc;
    return stage.finish();
}

}  // extern "C"
