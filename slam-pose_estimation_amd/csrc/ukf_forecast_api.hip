// ukf_forecast_api.hip -- C-ABI of the forecast (include/ukf_batch.h, "forecast"): argument checks (ukf_host.hpp), the one
// launch of a call, and the host-array form.
#include <vector>

#include "ukf_api_common.hpp"
#include "ukf_forecast_req.hpp"

namespace {

int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return ukfb::refuse_poisoned(e);
}

}  // namespace

extern "C" {

int ukfb_forecast_dev(ukfb_engine* e, int steps, const double* dt, const int64_t* ts_us, int slots, int first_slot,
                      const void* start_mu_dev, const void* start_cov_dev, const void* in_a_dev, const void* in_b_dev,
                      void* mu_out_dev, void* cov_out_dev, uint32_t* status_dev) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_forecast_args(steps, slots, first_slot, dt != nullptr, ts_us != nullptr, start_mu_dev != nullptr,
                                                            start_cov_dev != nullptr, mu_out_dev != nullptr)))
        return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    ukfb::ForecastReq r;
    r.steps = steps;
    r.slots = slots;
    r.first_slot = first_slot;
    r.dt = dt;   // copied into the kernel arguments: nothing of the caller's is read after the call returns
    r.ts_us = ts_us;
    r.start_mu_dev = start_mu_dev;
    r.start_cov_dev = start_cov_dev;
    r.in_a_dev = in_a_dev;
    r.in_b_dev = in_b_dev;
    r.mu_out_dev = mu_out_dev;
    r.cov_out_dev = cov_out_dev;
    r.status_dev = status_dev;
    return e->model == UKFB_MODEL_POSE ? ukfb::launch_forecast_pose(e, r) : ukfb::launch_forecast_orient(e, r);
}

int ukfb_forecast(ukfb_engine* e, int steps, const double* dt, const int64_t* ts_us, const double* start_mu,
                  const double* start_cov, const double* in_a, const double* in_b, double* mu, double* cov, uint32_t* status) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_forecast_args(steps, steps, 0, dt != nullptr, ts_us != nullptr, start_mu != nullptr,
                                                            start_cov != nullptr, mu != nullptr)))
        return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), ts = e->tsize, S = size_t(e->S), PK = size_t(e->PK), recs = size_t(steps) * n;
    ukfb::DeviceBuffers buf;
    void *mu_d = nullptr, *cov_d = nullptr, *a_d = nullptr, *b_d = nullptr, *smu_d = nullptr, *scov_d = nullptr;
    uint32_t* st_d = nullptr;
    UKFB_HIP_TRY(buf.take(&mu_d, recs * S * ts));
    if (cov) UKFB_HIP_TRY(buf.take(&cov_d, recs * PK * ts));
    if (start_mu) {
        UKFB_HIP_TRY(buf.take(&smu_d, n * S * ts));
        UKFB_HIP_TRY(buf.take(&scov_d, n * PK * ts));
    }
    if (in_a) UKFB_HIP_TRY(buf.take(&a_d, recs * 3 * ts));
    if (in_b) UKFB_HIP_TRY(buf.take(&b_d, recs * 3 * ts));
    if (status) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), n * sizeof(uint32_t)));
    std::vector<double> packed((cov ? recs : n) * PK);
    if (start_mu) {
        ukfb::pack_lower(start_cov, n, e->D, packed.data());
        if (const int rc = ukfb::upload_scalars(e, smu_d, start_mu, n * S)) return rc;
        if (const int rc = ukfb::upload_scalars(e, scov_d, packed.data(), n * PK)) return rc;
    }
    if (in_a)
        if (const int rc = ukfb::upload_scalars(e, a_d, in_a, recs * 3)) return rc;
    if (in_b)
        if (const int rc = ukfb::upload_scalars(e, b_d, in_b, recs * 3)) return rc;
    // an uninitialised filter's records are never written: they come back as zeros
    UKFB_HIP_TRY(hipMemsetAsync(mu_d, 0, recs * S * ts, ukfb::main_stream(e)));
    if (cov) UKFB_HIP_TRY(hipMemsetAsync(cov_d, 0, recs * PK * ts, ukfb::main_stream(e)));
    if (const int rc = ukfb_forecast_dev(e, steps, dt, ts_us, steps, 0, smu_d, scov_d, a_d, b_d, mu_d, cov_d, st_d)) return rc;
    if (const int rc = ukfb::download_scalars(e, mu_d, mu, recs * S)) return rc;
    if (cov) {
        if (const int rc = ukfb::download_scalars(e, cov_d, packed.data(), recs * PK)) return rc;
        ukfb::unpack_symmetric(packed.data(), recs, e->D, cov);
    }
    if (status) UKFB_HIP_TRY(hipMemcpyAsync(status, st_d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);   // (the temporaries are freed after the stream has drained)
}

}  // extern "C"
