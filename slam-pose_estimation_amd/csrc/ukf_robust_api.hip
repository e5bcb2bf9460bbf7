// ukf_robust_api.hip -- C-ABI of the robust sensor-frame update (include/ukf_batch_robust.h): argument checks
// (ukf_host.hpp), the device form and the host-array form.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

extern "C" {

int ukfb_update_robust_dev(ukfb_engine* e, int model_uniform, const ukfb_sensor_in* in, const ukfb_robust_rule* rule, int commit,
                           const ukfb_robust_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_robust_args(e->model, in && in->model_dev, model_uniform, in, rule, commit, out))) return rc;
    ON_DEVICE(e->device);
    ukfb::RobustReq r;
    r.model_uniform = model_uniform;
    r.in = *in;
    r.rule = *rule;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_update_robust(ukfb_engine* e, int model, const int32_t* model_per_filter, const double* z, const double* Q,
                       const double* mount, const double* mount_uniform, const double* point, const double* point_uniform,
                       const ukfb_robust_rule* rule, int commit, double* z_pred, double* S, double* innov, double* maha0,
                       double* maha, double* loglik, double* scale, int32_t* iterations, uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_sensor_in in{};
    in.model_dev = model_per_filter;
    in.z_dev = z;
    in.Q_dev = Q;
    in.mount_dev = mount;
    in.point_dev = point;
    ukfb::set_mount_point_uniform(&in, mount_uniform, point_uniform);
    const ukfb_robust_out wanted{z_pred, S, innov, maha0, maha, loglik, scale, iterations, status};
    if (const int rc = ukfb::fail(ukfb::check_robust_args(e->model, model_per_filter != nullptr, model, &in, rule, commit, &wanted))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap);
    ukfb::HostStage stage(e);
    in.model_dev = stage.raw_in(model_per_filter, n);
    in.z_dev = stage.in(z, n * 3);
    in.Q_dev = stage.in(Q, n * 9);
    in.mount_dev = stage.in(mount, n * 7);
    in.point_dev = stage.in(point, n * 3);
    ukfb_robust_out out{};
    out.z_pred = stage.out(z_pred, n * 3);
    out.S = stage.out(S, n * 9);
    out.innov = stage.out(innov, n * 3);
    out.maha0 = stage.out(maha0, n);
    out.maha = stage.out(maha, n);
    out.loglik = stage.out(loglik, n);
    out.scale = stage.out(scale, n);
    out.iterations = stage.raw_out(iterations, n);
    out.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_update_robust_dev(e, model, &in, rule, commit, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
