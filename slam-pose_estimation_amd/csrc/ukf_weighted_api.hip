// ukf_weighted_api.hip -- C-ABI of the sensor-frame update with given association weights (include/ukf_batch_jpda.h):
// argument checks (ukf_host.hpp), the device form and the host-array form.
#include "ukf_sensor_frame_api.hpp"

extern "C" {

int ukfb_update_weighted_dev(ukfb_engine* e, int model_uniform, const ukfb_associate_in* in, const void* weight_dev, int commit,
                             const ukfb_weighted_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_weighted_args(e->model, in && in->model_dev, model_uniform, in, weight_dev, commit, out))) return rc;
    ON_DEVICE(e->device);
    ukfb::WeightedReq r;
    r.model_uniform = model_uniform;
    r.in = *in;
    r.weight = weight_dev;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_update_weighted(ukfb_engine* e, int model, const int32_t* model_per_filter, int candidates, const double* z, const double* Q,
                         const double* mount, const double* mount_uniform, const double* point, const double* point_uniform,
                         const double* weight, int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik,
                         double* weight_used, double* beta0, double* innov_comb, int32_t* n_used, uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_associate_in in{};
    in.model_dev = model_per_filter;
    in.candidates = candidates;
    in.z_dev = z;
    in.Q_dev = Q;
    in.mount_dev = mount;
    in.point_dev = point;
    ukfb::set_mount_point_uniform(&in, mount_uniform, point_uniform);
    const ukfb_weighted_out wanted{z_pred, S, innov, maha, loglik, weight_used, beta0, innov_comb, n_used, status};
    if (const int rc = ukfb::fail(ukfb::check_weighted_args(e->model, model_per_filter != nullptr, model, &in, weight, commit, &wanted))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap);
    const size_t nz = size_t(ukfb::associate_out_scalars(candidates, e->cap, 3)), nk = size_t(ukfb::associate_out_scalars(candidates, e->cap, 1));
    ukfb::HostStage stage(e);
    in.model_dev = stage.raw_in(model_per_filter, n);
    in.z_dev = stage.in(z, nz);
    in.Q_dev = stage.in(Q, n * 9);
    in.mount_dev = stage.in(mount, n * 7);
    in.point_dev = stage.in(point, n * 3);
    const void* weight_dev = stage.in(weight, nk);
    ukfb_weighted_out out{};
    out.z_pred = stage.out(z_pred, n * 3);
    out.S = stage.out(S, n * 9);
    out.innov = stage.out(innov, nz);
    out.maha = stage.out(maha, nk);
    out.loglik = stage.out(loglik, nk);
    out.weight_used = stage.out(weight_used, nk);
    out.beta0 = stage.out(beta0, n);
    out.innov_comb = stage.out(innov_comb, n * 3);
    out.n_used = stage.raw_out(n_used, n);
    out.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_update_weighted_dev(e, model, &in, weight_dev, commit, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
