// ukf_condition_api.hip -- C-ABI of the covariance conditioning (include/ukf_batch.h, "covariance conditioning"): argument checks
// (ukf_host.hpp), the device form and the host-array form.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

extern "C" {

int ukfb_condition_dev(ukfb_engine* e, const ukfb_condition_in* in, int commit, const ukfb_condition_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_condition_args(in, commit, out))) return rc;
    ON_DEVICE(e->device);
    ukfb::ConditionReq r;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_condition(ukfb_engine* e, const double* var_floor, double eig_floor, const uint8_t* select, int renormalize_quaternion,
                   int commit, double* eig_min, double* eig_max, double* mu, double* cov, uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_condition_in in{};
    in.var_floor_dev = var_floor;
    in.eig_floor = eig_floor;
    in.select_dev = select;
    in.renormalize_quaternion = renormalize_quaternion;
    const ukfb_condition_out wanted{eig_min, eig_max, mu, cov, status};
    if (const int rc = ukfb::fail(ukfb::check_condition_args(&in, commit, &wanted))) return rc;
    if (const int rc = ukfb::fail(ukfb::check_condition_floor(var_floor, e->D))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap);
    ukfb::HostStage stage(e);
    in.var_floor_dev = stage.in(var_floor, size_t(e->D));
    in.select_dev = stage.raw_in(select, n);
    ukfb_condition_out out{};
    out.eig_min = stage.out(eig_min, n);
    out.eig_max = stage.out(eig_max, n);
    out.mu = stage.out(mu, n * size_t(e->S));
    out.cov_packed = stage.cov_out(cov, n);
    out.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_condition_dev(e, &in, commit, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
