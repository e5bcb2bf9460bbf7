// ukf_associate_api.hip -- C-ABI of the sensor-frame association (include/ukf_batch.h, "sensor-frame association"): argument
// checks (ukf_host.hpp), the device form and the host-array form.
#include <vector>

#include "ukf_api_common.hpp"
#include "ukf_associate_req.hpp"

namespace {

int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return ukfb::refuse_poisoned(e);
}

}  // namespace

extern "C" {

int ukfb_associate_sensor_dev(ukfb_engine* e, int model_uniform, const ukfb_associate_in* in, int commit, const ukfb_associate_out* out) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_associate_args(e->model, in && in->model_dev, model_uniform, in, commit, out))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    ukfb::AssociateReq r;
    r.model_uniform = model_uniform;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return e->model == UKFB_MODEL_POSE ? ukfb::launch_associate_pose(e, r) : ukfb::launch_associate_orient(e, r);
}

int ukfb_associate_sensor(ukfb_engine* e, int model, const int32_t* model_per_filter, int candidates, const double* z, const double* Q,
                          const double* mount, const double* mount_uniform, const double* point, const double* point_uniform,
                          int point_per_candidate, int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik,
                          int32_t* best, int32_t* n_gated, uint32_t* status) {
    if (const int rc = entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_associate_in in{};
    in.model_dev = model_per_filter;
    in.candidates = candidates;
    in.z_dev = z;
    in.Q_dev = Q;
    in.mount_dev = mount;
    in.point_dev = point;
    in.point_per_candidate = point_per_candidate;
    in.mount_uniform[6] = 1.0;   // r = 0, qs the identity, unless the caller says otherwise
    if (mount_uniform)
        for (int k = 0; k < 7; ++k) in.mount_uniform[k] = mount_uniform[k];
    if (point_uniform)
        for (int k = 0; k < 3; ++k) in.point_uniform[k] = point_uniform[k];
    ukfb_associate_out wanted{z_pred, S, innov, maha, loglik, best, n_gated, status};
    if (const int rc = ukfb::fail(ukfb::check_associate_args(e->model, model_per_filter != nullptr, model, &in, commit, &wanted))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    const size_t ts = e->tsize;
    const int64_t cap = e->cap;
    const int K = candidates, H = ukfb::associate_hypotheses(candidates, point_per_candidate);
    const size_t n = size_t(cap);
    const size_t nz = size_t(ukfb::associate_out_scalars(K, cap, 3)), nk = size_t(ukfb::associate_out_scalars(K, cap, 1));
    const size_t np = size_t(ukfb::associate_out_scalars(H, cap, 3)), nzp = np, ns = size_t(ukfb::associate_out_scalars(H, cap, 9));
    ukfb::DeviceBuffers buf;
    void *z_d = nullptr, *q_d = nullptr, *mount_d = nullptr, *point_d = nullptr;
    void *zp_d = nullptr, *s_d = nullptr, *inn_d = nullptr, *maha_d = nullptr, *ll_d = nullptr;
    int32_t *model_d = nullptr, *best_d = nullptr, *ng_d = nullptr;
    uint32_t* st_d = nullptr;
    UKFB_HIP_TRY(buf.take(&z_d, nz * ts));
    UKFB_HIP_TRY(buf.take(&q_d, n * 9 * ts));
    if (mount) UKFB_HIP_TRY(buf.take(&mount_d, n * 7 * ts));
    if (point) UKFB_HIP_TRY(buf.take(&point_d, np * ts));
    if (model_per_filter) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&model_d), n * sizeof(int32_t)));
    if (z_pred) UKFB_HIP_TRY(buf.take(&zp_d, nzp * ts));
    if (S) UKFB_HIP_TRY(buf.take(&s_d, ns * ts));
    if (innov) UKFB_HIP_TRY(buf.take(&inn_d, nz * ts));
    if (maha) UKFB_HIP_TRY(buf.take(&maha_d, nk * ts));
    if (loglik) UKFB_HIP_TRY(buf.take(&ll_d, nk * ts));
    if (best) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&best_d), n * sizeof(int32_t)));
    if (n_gated) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&ng_d), n * sizeof(int32_t)));
    if (status) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), n * sizeof(uint32_t)));
    if (const int rc = ukfb::upload_scalars(e, z_d, z, nz)) return rc;
    if (const int rc = ukfb::upload_scalars(e, q_d, Q, n * 9)) return rc;
    if (mount)
        if (const int rc = ukfb::upload_scalars(e, mount_d, mount, n * 7)) return rc;
    if (point)
        if (const int rc = ukfb::upload_scalars(e, point_d, point, np)) return rc;
    if (model_d) UKFB_HIP_TRY(hipMemcpyAsync(model_d, model_per_filter, n * sizeof(int32_t), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    in.model_dev = model_d;
    in.z_dev = z_d;
    in.Q_dev = q_d;
    in.mount_dev = mount_d;
    in.point_dev = point_d;
    const ukfb_associate_out out{zp_d, s_d, inn_d, maha_d, ll_d, best_d, ng_d, st_d};
    if (const int rc = ukfb_associate_sensor_dev(e, model, &in, commit, &out)) return rc;
    if (z_pred)
        if (const int rc = ukfb::download_scalars(e, zp_d, z_pred, nzp)) return rc;
    if (S)
        if (const int rc = ukfb::download_scalars(e, s_d, S, ns)) return rc;
    if (innov)
        if (const int rc = ukfb::download_scalars(e, inn_d, innov, nz)) return rc;
    if (maha)
        if (const int rc = ukfb::download_scalars(e, maha_d, maha, nk)) return rc;
    if (loglik)
        if (const int rc = ukfb::download_scalars(e, ll_d, loglik, nk)) return rc;
    if (best) UKFB_HIP_TRY(hipMemcpyAsync(best, best_d, n * sizeof(int32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    if (n_gated) UKFB_HIP_TRY(hipMemcpyAsync(n_gated, ng_d, n * sizeof(int32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    if (status) UKFB_HIP_TRY(hipMemcpyAsync(status, st_d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);   // (the temporaries are freed after the stream has drained)
}

}  // extern "C"
