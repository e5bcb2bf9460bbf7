// ukf_forecast_api.hip -- C-ABI of the forecast (include/ukf_batch.h, "forecast"): argument checks (ukf_host.hpp), the one
// launch of a call, and the host-array form.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

extern "C" {

int ukfb_forecast_dev(ukfb_engine* e, int steps, const double* dt, const int64_t* ts_us, int slots, int first_slot,
                      const void* start_mu_dev, const void* start_cov_dev, const void* in_a_dev, const void* in_b_dev,
                      void* mu_out_dev, void* cov_out_dev, uint32_t* status_dev) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_forecast_args(steps, slots, first_slot, dt != nullptr, ts_us != nullptr, start_mu_dev != nullptr,
                                                            start_cov_dev != nullptr, mu_out_dev != nullptr)))
        return rc;
    ON_DEVICE(e->device);
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
    return ukfb::launch_for_model(e, r);
}

int ukfb_forecast(ukfb_engine* e, int steps, const double* dt, const int64_t* ts_us, const double* start_mu,
                  const double* start_cov, const double* in_a, const double* in_b, double* mu, double* cov, uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_forecast_args(steps, steps, 0, dt != nullptr, ts_us != nullptr, start_mu != nullptr,
                                                            start_cov != nullptr, mu != nullptr)))
        return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), S = size_t(e->S), recs = size_t(steps) * n;
    ukfb::HostStage stage(e);
    const void* smu_d = stage.in(start_mu, n * S);
    const void* scov_d = stage.cov_in(start_cov, n);
    const void* a_d = stage.in(in_a, recs * 3);
    const void* b_d = stage.in(in_b, recs * 3);
    // an uninitialised filter's records are never written: they come back as zeros
    void* mu_d = stage.out(mu, recs * S, true);
    void* cov_d = stage.cov_out(cov, recs, true);
    uint32_t* st_d = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_forecast_dev(e, steps, dt, ts_us, steps, 0, smu_d, scov_d, a_d, b_d, mu_d, cov_d, st_d)) return rc;
    return stage.finish();
}

}  // extern "C"
