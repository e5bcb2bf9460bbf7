// ukf_delayed_api.hip -- C-ABI of the delayed-measurement update (include/ukf_batch.h, "late samples"): argument checks
// (ukf_host.hpp), the device form, the lag helper and the host-array form.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

namespace ukfb {

// ukfb_delayed_lag_dev: one thread per filter, the window's stamps by value
struct DelayedLagArgs {
    int64_t n;
    int steps;
    const int64_t* sample_ts;
    int32_t* lag_out;
    int64_t step_ts[DELAYED_MAX_STEPS];
};
__global__ void delayed_lag_kernel(const DelayedLagArgs a) {
    const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i >= a.n) return;
    a.lag_out[i] = delayed_lag_of(a.steps, a.step_ts, a.sample_ts[i]);
}

}  // namespace ukfb

extern "C" {

int ukfb_update_delayed_dev(ukfb_engine* e, const ukfb_delayed_in* in, int commit, const ukfb_delayed_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_delayed_args(in, commit, out))) return rc;
    ON_DEVICE(e->device);
    ukfb::DelayedReq r;
    r.in = *in;   // (in->dt is copied into the kernel arguments: nothing of the caller's is read after the call returns)
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_delayed_lag_dev(ukfb_engine* e, int steps, const int64_t* step_ts_us, const int64_t* sample_ts_us_dev, int32_t* lag_out_dev) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_delayed_lag_args(steps, step_ts_us, sample_ts_us_dev != nullptr, lag_out_dev != nullptr)))
        return rc;
    ON_DEVICE(e->device);
    if (e->cap == 0) return UKFB_OK;
    ukfb::DelayedLagArgs a{};
    a.n = e->cap;
    a.steps = steps;
    a.sample_ts = sample_ts_us_dev;
    a.lag_out = lag_out_dev;
    for (int c = 0; c < steps; ++c) a.step_ts[c] = step_ts_us[c];
    const unsigned grid = unsigned((e->cap + 255) / 256);
    hipLaunchKernelGGL(ukfb::delayed_lag_kernel, dim3(grid), dim3(256), 0, ukfb::main_stream(e), a);
    return ukfb::launch_status("delayed-lag kernel launch");
}

int ukfb_update_delayed(ukfb_engine* e, int steps, const double* dt, const double* mu_hist, const double* cov_hist, const double* in_a,
                        const double* in_b, int lag_uniform, const int32_t* lag, int meas_model, const int32_t* meas_model_per_filter,
                        const double* z, const double* Q, int commit, double* z_pred, double* S, double* innov, double* maha,
                        double* loglik, uint32_t* status, double* mu_out, double* cov_out) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_delayed_in in{};
    in.steps = steps;
    in.dt = dt;
    in.slots = steps;
    in.first_slot = 0;
    in.mu_hist_dev = mu_hist;
    in.cov_hist_dev = cov_hist;
    in.lag_uniform = lag_uniform;
    in.meas_model_uniform = meas_model;
    in.z_dev = z;
    in.Q_dev = Q;
    const ukfb_delayed_out wanted{z_pred, S, innov, maha, loglik, status, mu_out, cov_out};
    if (const int rc = ukfb::fail(ukfb::check_delayed_args(&in, commit, &wanted))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), SS = size_t(e->S), recs = size_t(steps) * n;
    ukfb::HostStage stage(e);
    in.mu_hist_dev = stage.in(mu_hist, recs * SS);
    in.cov_hist_dev = stage.cov_in(cov_hist, recs);
    in.in_a_dev = stage.in(in_a, recs * 3);
    in.in_b_dev = stage.in(in_b, recs * 3);
    in.lag_dev = stage.raw_in(lag, n);
    in.meas_model_dev = stage.raw_in(meas_model_per_filter, n);
    in.z_dev = stage.in(z, n * 3);
    in.Q_dev = stage.in(Q, n * 9);
    ukfb_delayed_out out{};
    out.z_pred = stage.out(z_pred, n * 4);
    out.S = stage.out(S, n * 9);
    out.innov = stage.out(innov, n * 3);
    out.maha = stage.out(maha, n);
    out.loglik = stage.out(loglik, n);
    out.status = stage.raw_out(status, n);
    out.mu_out = stage.out(mu_out, n * SS);
    out.cov_out = stage.cov_out(cov_out, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_update_delayed_dev(e, &in, commit, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
