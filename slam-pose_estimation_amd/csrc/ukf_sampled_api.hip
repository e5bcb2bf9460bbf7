// ukf_sampled_api.hip -- C-ABI of the user-defined measurement models (include/ukf_batch.h, "user-defined measurement models"):
// argument checks (ukf_host.hpp), the device forms and the host-array forms.
#include <vector>

#include "ukf_api_common.hpp"
#include "ukf_sampled_req.hpp"

namespace {

int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return ukfb::refuse_poisoned(e);
}

}  // namespace

extern "C" {

int ukfb_sigma_points_dev(ukfb_engine* e, void* X_out_dev, void* delta_out_dev, uint32_t* status_dev) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_sigma_points_args(X_out_dev != nullptr, delta_out_dev != nullptr))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    ukfb::SigmaPointsReq r;
    r.X = X_out_dev;
    r.delta = delta_out_dev;
    r.status = status_dev;
    return e->model == UKFB_MODEL_POSE ? ukfb::launch_sigma_points_pose(e, r) : ukfb::launch_sigma_points_orient(e, r);
}

int ukfb_update_sampled_dev(ukfb_engine* e, const ukfb_sampled_in* in, int commit, const ukfb_sampled_out* out) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_sampled_args(in, commit, out))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    ukfb::SampledReq r;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return e->model == UKFB_MODEL_POSE ? ukfb::launch_sampled_pose(e, r) : ukfb::launch_sampled_orient(e, r);
}

int ukfb_sigma_points(ukfb_engine* e, double* X, double* delta, uint32_t* status) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_sigma_points_args(X != nullptr, delta != nullptr))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), ts = e->tsize, pts = size_t(ukfb::sampled_points(e->D));
    ukfb::DeviceBuffers buf;
    void *x_d = nullptr, *d_d = nullptr;
    uint32_t* st_d = nullptr;
    if (X) UKFB_HIP_TRY(buf.take(&x_d, n * pts * size_t(e->S) * ts));
    if (delta) UKFB_HIP_TRY(buf.take(&d_d, n * pts * size_t(e->D) * ts));
    if (status) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), n * sizeof(uint32_t)));
    if (const int rc = ukfb_sigma_points_dev(e, x_d, d_d, st_d)) return rc;
    if (X)
        if (const int rc = ukfb::download_scalars(e, x_d, X, n * pts * size_t(e->S))) return rc;
    if (delta)
        if (const int rc = ukfb::download_scalars(e, d_d, delta, n * pts * size_t(e->D))) return rc;
    if (status) UKFB_HIP_TRY(hipMemcpyAsync(status, st_d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);   // (the temporaries are freed after the stream has drained)
}

int ukfb_update_sampled(ukfb_engine* e, int m, const double* Z, const double* z, const double* Q, int q_is_uniform,
                        const uint8_t* active, int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik,
                        uint32_t* status) {
    if (const int rc = entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_sampled_in in{};
    in.m = m;
    in.Z_dev = Z;
    in.z_dev = z;
    in.Q_dev = Q;
    in.q_is_uniform = q_is_uniform;
    in.active_dev = active;
    ukfb_sampled_out wanted{z_pred, S, innov, maha, loglik, status};
    if (const int rc = ukfb::fail(ukfb::check_sampled_args(&in, commit, &wanted))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), ts = e->tsize, mz = size_t(m), pts = size_t(ukfb::sampled_points(e->D));
    const size_t nq = (q_is_uniform ? size_t(1) : n) * mz * mz;
    ukfb::DeviceBuffers buf;
    void *Z_d = nullptr, *z_d = nullptr, *q_d = nullptr, *act_d = nullptr;
    void *zp_d = nullptr, *s_d = nullptr, *inn_d = nullptr, *maha_d = nullptr, *ll_d = nullptr;
    uint32_t* st_d = nullptr;
    UKFB_HIP_TRY(buf.take(&Z_d, n * pts * mz * ts));
    UKFB_HIP_TRY(buf.take(&z_d, n * mz * ts));
    UKFB_HIP_TRY(buf.take(&q_d, nq * ts));
    if (active) UKFB_HIP_TRY(buf.take(&act_d, n));
    if (z_pred) UKFB_HIP_TRY(buf.take(&zp_d, n * mz * ts));
    if (S) UKFB_HIP_TRY(buf.take(&s_d, n * mz * mz * ts));
    if (innov) UKFB_HIP_TRY(buf.take(&inn_d, n * mz * ts));
    if (maha) UKFB_HIP_TRY(buf.take(&maha_d, n * ts));
    if (loglik) UKFB_HIP_TRY(buf.take(&ll_d, n * ts));
    if (status) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), n * sizeof(uint32_t)));
    if (const int rc = ukfb::upload_scalars(e, Z_d, Z, n * pts * mz)) return rc;
    if (const int rc = ukfb::upload_scalars(e, z_d, z, n * mz)) return rc;
    if (const int rc = ukfb::upload_scalars(e, q_d, Q, nq)) return rc;
    if (active) UKFB_HIP_TRY(hipMemcpyAsync(act_d, active, n, hipMemcpyHostToDevice, ukfb::main_stream(e)));
    in.Z_dev = Z_d;
    in.z_dev = z_d;
    in.Q_dev = q_d;
    in.active_dev = static_cast<const uint8_t*>(act_d);
    const ukfb_sampled_out out{zp_d, s_d, inn_d, maha_d, ll_d, st_d};
    if (const int rc = ukfb_update_sampled_dev(e, &in, commit, &out)) return rc;
    if (z_pred)
        if (const int rc = ukfb::download_scalars(e, zp_d, z_pred, n * mz)) return rc;
    if (S)
        if (const int rc = ukfb::download_scalars(e, s_d, S, n * mz * mz)) return rc;
    if (innov)
        if (const int rc = ukfb::download_scalars(e, inn_d, innov, n * mz)) return rc;
    if (maha)
        if (const int rc = ukfb::download_scalars(e, maha_d, maha, n)) return rc;
    if (loglik)
        if (const int rc = ukfb::download_scalars(e, ll_d, loglik, n)) return rc;
    if (status) UKFB_HIP_TRY(hipMemcpyAsync(status, st_d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);   // (the temporaries are freed after the stream has drained)
}

}  // extern "C"
