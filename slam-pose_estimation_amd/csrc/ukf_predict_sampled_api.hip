// ukf_predict_sampled_api.hip -- C-ABI of the user-defined process models (include/ukf_batch.h, "user-defined process models"):
// argument checks (ukf_host.hpp), the device form and the host-array form.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

extern "C" {

int ukfb_predict_sampled_dev(ukfb_engine* e, const ukfb_predict_sampled_in* in, int commit, const ukfb_predict_sampled_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_predict_sampled_args(in, commit, out))) return rc;
    ON_DEVICE(e->device);
    ukfb::PredictSampledReq r;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_predict_sampled(ukfb_engine* e, const double* XX, const double* R, int r_is_uniform, const uint8_t* active, int commit,
                         double* mu, double* cov, uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_predict_sampled_in in{};
    in.XX_dev = XX;
    in.R_dev = R;
    in.r_is_uniform = r_is_uniform;
    in.active_dev = active;
    const ukfb_predict_sampled_out wanted{mu, cov, status};
    if (const int rc = ukfb::fail(ukfb::check_predict_sampled_args(&in, commit, &wanted))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), S = size_t(e->S), D = size_t(e->D), pts = size_t(ukfb::sampled_points(e->D));
    ukfb::HostStage stage(e);
    in.XX_dev = stage.in(XX, n * pts * S);
    in.R_dev = stage.in(R, (r_is_uniform ? size_t(1) : n) * D * D);
    in.active_dev = stage.raw_in(active, n);
    ukfb_predict_sampled_out out{};
    out.mu = stage.out(mu, n * S);
    out.cov_packed = stage.cov_out(cov, n);
    out.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_predict_sampled_dev(e, &in, commit, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
