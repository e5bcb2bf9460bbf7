// ukf_bearing_api.hip -- C-ABI of the bearing measurements (include/ukf_batch.h, "bearing measurements"):
// argument checks (ukf_host.hpp), the device form and the host-array form.
#include <vector>

#include "ukf_api_common.hpp"
#include "ukf_bearing_req.hpp"

namespace {

int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return ukfb::refuse_poisoned(e);
}

}  // namespace

extern "C" {

int ukfb_update_bearing_dev(ukfb_engine* e, int model_uniform, const ukfb_sensor_in* in, int commit, const ukfb_sensor_out* out) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_bearing_args(e->model, in && in->model_dev, model_uniform, in, commit, out))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    ukfb::BearingReq r;
    r.model_uniform = model_uniform;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return e->model == UKFB_MODEL_POSE ? ukfb::launch_bearing_pose(e, r) : ukfb::launch_bearing_orient(e, r);
}

int ukfb_update_bearing(ukfb_engine* e, int model, const int32_t* model_per_filter, const double* z, const double* Q, const double* mount,
                       const double* mount_uniform, const double* point, const double* point_uniform, int commit, double* z_pred,
                       double* S, double* innov, double* maha, double* loglik, uint32_t* status) {
    if (const int rc = entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_sensor_in in{};
    in.model_dev = model_per_filter;
    in.z_dev = z;
    in.Q_dev = Q;
    in.mount_dev = mount;
    in.point_dev = point;
    in.mount_uniform[6] = 1.0;   // r = 0, qs the identity, unless the caller says otherwise
    if (mount_uniform)
        for (int k = 0; k < 7; ++k) in.mount_uniform[k] = mount_uniform[k];
    if (point_uniform)
        for (int k = 0; k < 3; ++k) in.point_uniform[k] = point_uniform[k];
    ukfb_sensor_out wanted{z_pred, S, innov, maha, loglik, status};
    if (const int rc = ukfb::fail(ukfb::check_bearing_args(e->model, model_per_filter != nullptr, model, &in, commit, &wanted))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), ts = e->tsize;
    ukfb::DeviceBuffers buf;
    void *z_d = nullptr, *q_d = nullptr, *mount_d = nullptr, *point_d = nullptr;
    void *zp_d = nullptr, *s_d = nullptr, *inn_d = nullptr, *maha_d = nullptr, *ll_d = nullptr;
    int32_t* model_d = nullptr;
    uint32_t* st_d = nullptr;
    UKFB_HIP_TRY(buf.take(&z_d, n * 3 * ts));
    UKFB_HIP_TRY(buf.take(&q_d, n * 9 * ts));
    if (mount) UKFB_HIP_TRY(buf.take(&mount_d, n * 7 * ts));
    if (point) UKFB_HIP_TRY(buf.take(&point_d, n * 3 * ts));
    if (model_per_filter) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&model_d), n * sizeof(int32_t)));
    if (z_pred) UKFB_HIP_TRY(buf.take(&zp_d, n * 3 * ts));
    if (S) UKFB_HIP_TRY(buf.take(&s_d, n * 9 * ts));
    if (innov) UKFB_HIP_TRY(buf.take(&inn_d, n * 3 * ts));
    if (maha) UKFB_HIP_TRY(buf.take(&maha_d, n * ts));
    if (loglik) UKFB_HIP_TRY(buf.take(&ll_d, n * ts));
    if (status) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), n * sizeof(uint32_t)));
    if (const int rc = ukfb::upload_scalars(e, z_d, z, n * 3)) return rc;
    if (const int rc = ukfb::upload_scalars(e, q_d, Q, n * 9)) return rc;
    if (mount)
        if (const int rc = ukfb::upload_scalars(e, mount_d, mount, n * 7)) return rc;
    if (point)
        if (const int rc = ukfb::upload_scalars(e, point_d, point, n * 3)) return rc;
    if (model_d) UKFB_HIP_TRY(hipMemcpyAsync(model_d, model_per_filter, n * sizeof(int32_t), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    in.model_dev = model_d;
    in.z_dev = z_d;
    in.Q_dev = q_d;
    in.mount_dev = mount_d;
    in.point_dev = point_d;
    const ukfb_sensor_out out{zp_d, s_d, inn_d, maha_d, ll_d, st_d};
    if (const int rc = ukfb_update_bearing_dev(e, model, &in, commit, &out)) return rc;
    if (z_pred)
        if (const int rc = ukfb::download_scalars(e, zp_d, z_pred, n * 3)) return rc;
    if (S)
        if (const int rc = ukfb::download_scalars(e, s_d, S, n * 9)) return rc;
    if (innov)
        if (const int rc = ukfb::download_scalars(e, inn_d, innov, n * 3)) return rc;
    if (maha)
        if (const int rc = ukfb::download_scalars(e, maha_d, maha, n)) return rc;
    if (loglik)
        if (const int rc = ukfb::download_scalars(e, ll_d, loglik, n)) return rc;
    if (status) UKFB_HIP_TRY(hipMemcpyAsync(status, st_d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);   // (the temporaries are freed after the stream has drained)
}

}  // extern "C"
