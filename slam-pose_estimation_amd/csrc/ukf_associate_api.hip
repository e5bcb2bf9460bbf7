// ukf_associate_api.hip -- C-ABI of the sensor-frame association (include/ukf_batch.h, "sensor-frame association"): argument
// checks (ukf_host.hpp), the device form and the host-array form.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

extern "C" {

int ukfb_associate_sensor_dev(ukfb_engine* e, int model_uniform, const ukfb_associate_in* in, int commit, const ukfb_associate_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_associate_args(e->model, in && in->model_dev, model_uniform, in, commit, out))) return rc;
    ON_DEVICE(e->device);
    ukfb::AssociateReq r;
    r.model_uniform = model_uniform;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_associate_sensor(ukfb_engine* e, int model, const int32_t* model_per_filter, int candidates, const double* z, const double* Q,
                          const double* mount, const double* mount_uniform, const double* point, const double* point_uniform,
                          int point_per_candidate, int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik,
                          int32_t* best, int32_t* n_gated, uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_associate_in in{};
    in.model_dev = model_per_filter;
    in.candidates = candidates;
    in.z_dev = z;
    in.Q_dev = Q;
    in.mount_dev = mount;
    in.point_dev = point;
    in.point_per_candidate = point_per_candidate;
    ukfb::set_mount_point_uniform(&in, mount_uniform, point_uniform);
    const ukfb_associate_out wanted{z_pred, S, innov, maha, loglik, best, n_gated, status};
    if (const int rc = ukfb::fail(ukfb::check_associate_args(e->model, model_per_filter != nullptr, model, &in, commit, &wanted))) return rc;
    ON_DEVICE(e->device);
    const int K = candidates, H = ukfb::associate_hypotheses(candidates, point_per_candidate);
    const size_t n = size_t(e->cap);
    const size_t nz = size_t(ukfb::associate_out_scalars(K, e->cap, 3)), nk = size_t(ukfb::associate_out_scalars(K, e->cap, 1));
    const size_t np = size_t(ukfb::associate_out_scalars(H, e->cap, 3)), ns = size_t(ukfb::associate_out_scalars(H, e->cap, 9));
    ukfb::HostStage stage(e);
    in.model_dev = stage.raw_in(model_per_filter, n);
    in.z_dev = stage.in(z, nz);
    in.Q_dev = stage.in(Q, n * 9);
    in.mount_dev = stage.in(mount, n * 7);
    in.point_dev = stage.in(point, np);
    ukfb_associate_out out{};
    out.z_pred = stage.out(z_pred, np);
    out.S = stage.out(S, ns);
    out.innov = stage.out(innov, nz);
    out.maha = stage.out(maha, nk);
    out.loglik = stage.out(loglik, nk);
    out.best = stage.raw_out(best, n);
    out.n_gated = stage.raw_out(n_gated, n);
    out.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_associate_sensor_dev(e, model, &in, commit, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
