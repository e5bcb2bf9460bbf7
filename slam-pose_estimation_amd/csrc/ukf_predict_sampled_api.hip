// ukf_predict_sampled_api.hip -- C-ABI of the user-defined process models (include/ukf_batch.h, "user-defined process models"):
// argument checks (ukf_host.hpp), the device form and the host-array form.
#include <vector>

#include "ukf_api_common.hpp"
#include "ukf_predict_sampled_req.hpp"

namespace {

int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return ukfb::refuse_poisoned(e);
}

}  // namespace

extern "C" {

int ukfb_predict_sampled_dev(ukfb_engine* e, const ukfb_predict_sampled_in* in, int commit, const ukfb_predict_sampled_out* out) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_predict_sampled_args(in, commit, out))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    ukfb::PredictSampledReq r;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return e->model == UKFB_MODEL_POSE ? ukfb::launch_predict_sampled_pose(e, r) : ukfb::launch_predict_sampled_orient(e, r);
}

int ukfb_predict_sampled(ukfb_engine* e, const double* XX, const double* R, int r_is_uniform, const uint8_t* active, int commit,
                         double* mu, double* cov, uint32_t* status) {
    if (const int rc = entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_predict_sampled_in in{};
    in.XX_dev = XX;
    in.R_dev = R;
    in.r_is_uniform = r_is_uniform;
    in.active_dev = active;
    const ukfb_predict_sampled_out wanted{mu, cov, status};
    if (const int rc = ukfb::fail(ukfb::check_predict_sampled_args(&in, commit, &wanted))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), ts = e->tsize, S = size_t(e->S), D = size_t(e->D), PK = size_t(e->PK);
    const size_t pts = size_t(ukfb::sampled_points(e->D)), nr = (r_is_uniform ? size_t(1) : n) * D * D;
    ukfb::DeviceBuffers buf;
    void *xx_d = nullptr, *r_d = nullptr, *act_d = nullptr, *mu_d = nullptr, *cov_d = nullptr;
    uint32_t* st_d = nullptr;
    UKFB_HIP_TRY(buf.take(&xx_d, n * pts * S * ts));
    UKFB_HIP_TRY(buf.take(&r_d, nr * ts));
    if (active) UKFB_HIP_TRY(buf.take(&act_d, n));
    if (mu) UKFB_HIP_TRY(buf.take(&mu_d, n * S * ts));
    if (cov) UKFB_HIP_TRY(buf.take(&cov_d, n * PK * ts));
    if (status) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), n * sizeof(uint32_t)));
    if (const int rc = ukfb::upload_scalars(e, xx_d, XX, n * pts * S)) return rc;
    if (const int rc = ukfb::upload_scalars(e, r_d, R, nr)) return rc;
    if (active) UKFB_HIP_TRY(hipMemcpyAsync(act_d, active, n, hipMemcpyHostToDevice, ukfb::main_stream(e)));
    in.XX_dev = xx_d;
    in.R_dev = r_d;
    in.active_dev = static_cast<const uint8_t*>(act_d);
    const ukfb_predict_sampled_out out{mu_d, cov_d, st_d};
    if (const int rc = ukfb_predict_sampled_dev(e, &in, commit, &out)) return rc;
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
