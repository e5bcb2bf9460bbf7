// ukf_sampled_api.hip -- C-ABI of the user-defined measurement models (include/ukf_batch.h, "user-defined measurement models"):
// argument checks (ukf_host.hpp), the device forms and the host-array forms.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

extern "C" {

int ukfb_sigma_points_dev(ukfb_engine* e, void* X_out_dev, void* delta_out_dev, uint32_t* status_dev) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_sigma_points_args(X_out_dev != nullptr, delta_out_dev != nullptr))) return rc;
    ON_DEVICE(e->device);
    ukfb::SigmaPointsReq r;
    r.X = X_out_dev;
    r.delta = delta_out_dev;
    r.status = status_dev;
    return ukfb::launch_for_model(e, r);
}

int ukfb_update_sampled_dev(ukfb_engine* e, const ukfb_sampled_in* in, int commit, const ukfb_sampled_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_sampled_args(in, commit, out))) return rc;
    ON_DEVICE(e->device);
    ukfb::SampledReq r;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_sigma_points(ukfb_engine* e, double* X, double* delta, uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_sigma_points_args(X != nullptr, delta != nullptr))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), pts = size_t(ukfb::sampled_points(e->D));
    ukfb::HostStage stage(e);
    void* x_d = stage.out(X, n * pts * size_t(e->S));
    void* d_d = stage.out(delta, n * pts * size_t(e->D));
    uint32_t* st_d = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_sigma_points_dev(e, x_d, d_d, st_d)) return rc;
    return stage.finish();
}

int ukfb_update_sampled(ukfb_engine* e, int m, const double* Z, const double* z, const double* Q, int q_is_uniform,
                        const uint8_t* active, int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik,
                        uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_sampled_in in{};
    in.m = m;
    in.Z_dev = Z;
    in.z_dev = z;
    in.Q_dev = Q;
    in.q_is_uniform = q_is_uniform;
    in.active_dev = active;
    const ukfb_sampled_out wanted{z_pred, S, innov, maha, loglik, status};
    if (const int rc = ukfb::fail(ukfb::check_sampled_args(&in, commit, &wanted))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), mz = size_t(m), pts = size_t(ukfb::sampled_points(e->D));
    ukfb::HostStage stage(e);
    in.Z_dev = stage.in(Z, n * pts * mz);
    in.z_dev = stage.in(z, n * mz);
    in.Q_dev = stage.in(Q, (q_is_uniform ? size_t(1) : n) * mz * mz);
    in.active_dev = stage.raw_in(active, n);
    ukfb_sampled_out out{};
    out.z_pred = stage.out(z_pred, n * mz);
    out.S = stage.out(S, n * mz * mz);
    out.innov = stage.out(innov, n * mz);
    out.maha = stage.out(maha, n);
    out.loglik = stage.out(loglik, n);
    out.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_update_sampled_dev(e, &in, commit, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
