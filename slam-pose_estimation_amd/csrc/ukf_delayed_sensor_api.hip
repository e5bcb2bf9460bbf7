// ukf_delayed_sensor_api.hip -- C-ABI of the late sensor-frame samples (include/ukf_batch_delayed_sensor.h): argument checks
// (ukf_host.hpp), the device form and the host-array form.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

extern "C" {

int ukfb_update_delayed_sensor_dev(ukfb_engine* e, const ukfb_delayed_sensor_in* in, int commit, const ukfb_delayed_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_delayed_sensor_args(e->model, in, commit, out))) return rc;
    ON_DEVICE(e->device);
    ukfb::DelayedSensorReq r;
    r.in = *in;   // (in->dt is copied into the kernel arguments: nothing of the caller's is read after the call returns)
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_update_delayed_sensor(ukfb_engine* e, int steps, const double* dt, const double* mu_hist, const double* cov_hist,
                               const double* in_a, const double* in_b, int lag_uniform, const int32_t* lag, int model,
                               const int32_t* model_per_filter, const double* z, const double* Q, const double* mount,
                               const double* mount_uniform, const double* point, const double* point_uniform, const double* rate,
                               int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik, uint32_t* status,
                               double* mu_out, double* cov_out) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_delayed_sensor_in in{};
    in.steps = steps;
    in.dt = dt;
    in.slots = steps;
    in.first_slot = 0;
    in.mu_hist_dev = mu_hist;
    in.cov_hist_dev = cov_hist;
    in.lag_uniform = lag_uniform;
    in.model_uniform = model;
    in.model_dev = model_per_filter;
    in.z_dev = z;
    in.Q_dev = Q;
    ukfb::set_mount_point_uniform(&in, mount_uniform, point_uniform);
    const ukfb_delayed_out wanted{z_pred, S, innov, maha, loglik, status, mu_out, cov_out};
    if (const int rc = ukfb::fail(ukfb::check_delayed_sensor_args(e->model, &in, commit, &wanted))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), SS = size_t(e->S), recs = size_t(steps) * n;
    ukfb::HostStage stage(e);
    in.mu_hist_dev = stage.in(mu_hist, recs * SS);
    in.cov_hist_dev = stage.cov_in(cov_hist, recs);
    in.in_a_dev = stage.in(in_a, recs * 3);
    in.in_b_dev = stage.in(in_b, recs * 3);
    in.lag_dev = stage.raw_in(lag, n);
    in.model_dev = stage.raw_in(model_per_filter, n);
    in.z_dev = stage.in(z, n * 3);
    in.Q_dev = stage.in(Q, n * 9);
    in.mount_dev = stage.in(mount, n * 7);
    in.point_dev = stage.in(point, n * 3);
    in.rate_dev = stage.in(rate, n * 3);
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
    if (const int rc = ukfb_update_delayed_sensor_dev(e, &in, commit, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
