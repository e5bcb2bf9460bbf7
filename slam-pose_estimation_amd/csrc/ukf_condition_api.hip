// ukf_condition_api.hip -- C-ABI of the covariance conditioning (include/ukf_batch.h, "covariance conditioning"): argument checks
// (ukf_host.hpp), the device form and the host-array form.
#include <vector>

#include "ukf_api_common.hpp"
#include "ukf_condition_req.hpp"

namespace {

int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return ukfb::refuse_poisoned(e);
}

}  // namespace

extern "C" {

int ukfb_condition_dev(ukfb_engine* e, const ukfb_condition_in* in, int commit, const ukfb_condition_out* out) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_condition_args(in, commit, out))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    ukfb::ConditionReq r;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return e->model == UKFB_MODEL_POSE ? ukfb::launch_condition_pose(e, r) : ukfb::launch_condition_orient(e, r);
}

int ukfb_condition(ukfb_engine* e, const double* var_floor, double eig_floor, const uint8_t* select, int renormalize_quaternion,
                   int commit, double* eig_min, double* eig_max, double* mu, double* cov, uint32_t* status) {
    if (const int rc = entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_condition_in in{};
    in.var_floor_dev = var_floor;
    in.eig_floor = eig_floor;
    in.select_dev = select;
    in.renormalize_quaternion = renormalize_quaternion;
    const ukfb_condition_out wanted{eig_min, eig_max, mu, cov, status};
    if (const int rc = ukfb::fail(ukfb::check_condition_args(&in, commit, &wanted))) return rc;
    if (const int rc = ukfb::fail(ukfb::check_condition_floor(var_floor, e->D))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), ts = e->tsize, S = size_t(e->S), D = size_t(e->D), PK = size_t(e->PK);
    ukfb::DeviceBuffers buf;
    void *fl_d = nullptr, *sel_d = nullptr, *lo_d = nullptr, *hi_d = nullptr, *mu_d = nullptr, *cov_d = nullptr;
    uint32_t* st_d = nullptr;
    UKFB_HIP_TRY(buf.take(&fl_d, D * ts));
    if (select) UKFB_HIP_TRY(buf.take(&sel_d, n));
    if (eig_min) UKFB_HIP_TRY(buf.take(&lo_d, n * ts));
    if (eig_max) UKFB_HIP_TRY(buf.take(&hi_d, n * ts));
    if (mu) UKFB_HIP_TRY(buf.take(&mu_d, n * S * ts));
    if (cov) UKFB_HIP_TRY(buf.take(&cov_d, n * PK * ts));
    if (status) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), n * sizeof(uint32_t)));
    if (const int rc = ukfb::upload_scalars(e, fl_d, var_floor, D)) return rc;
    if (select) UKFB_HIP_TRY(hipMemcpyAsync(sel_d, select, n, hipMemcpyHostToDevice, ukfb::main_stream(e)));
    in.var_floor_dev = fl_d;
    in.select_dev = static_cast<const uint8_t*>(sel_d);
    const ukfb_condition_out out{lo_d, hi_d, mu_d, cov_d, st_d};
    if (const int rc = ukfb_condition_dev(e, &in, commit, &out)) return rc;
    if (eig_min)
        if (const int rc = ukfb::download_scalars(e, lo_d, eig_min, n)) return rc;
    if (eig_max)
        if (const int rc = ukfb::download_scalars(e, hi_d, eig_max, n)) return rc;
    if (mu)
        if (const int rc = ukfb::download_scalars(e, mu_d, mu, n * S)) return rc;
    if (cov) {
        std::vector<double> packed(n * PK);
        if (const int rc = ukfb::download_scalars(e, cov_d, packed.data(), n * PK)) return rc;
        ukfb::unpack_symmetric(packed.data(), n, e->D, cov);
    }
    if (status) UKFB_HIP_TRY(hipMemcpyAsync(status, st_d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);   // (the temporaries are freed after the stream has drained)
}

}  // extern "C"
