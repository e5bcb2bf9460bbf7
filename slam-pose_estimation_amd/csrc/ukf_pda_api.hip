// ukf_pda_api.hip -- C-ABI of the probabilistic data association update (include/ukf_batch_pda.h): argument checks
// (ukf_host.hpp), the device form and the host-array form.
#include "ukf_sensor_frame_api.hpp"

extern "C" {

int ukfb_update_pda_dev(ukfb_engine* e, int model_uniform, const ukfb_associate_in* in, const ukfb_pda_rule* rule, int commit,
                        const ukfb_pda_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_pda_args(e->model, in && in->model_dev, model_uniform, in, rule, commit, out))) return rc;
    ON_DEVICE(e->device);
    ukfb::PdaReq r;
    r.model_uniform = model_uniform;
    r.in = *in;
    r.rule = *rule;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_update_pda(ukfb_engine* e, int model, const int32_t* model_per_filter, int candidates, const double* z, const double* Q,
                    const double* mount, const double* mount_uniform, const double* point, const double* point_uniform,
                    const ukfb_pda_rule* rule, int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik,
                    double* beta, double* beta0, double* innov_comb, int32_t* best, int32_t* n_gated, uint32_t* status) {
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
    const ukfb_pda_out wanted{z_pred, S, innov, maha, loglik, beta, beta0, innov_comb, best, n_gated, status};
    if (const int rc = ukfb::fail(ukfb::check_pda_args(e->model, model_per_filter != nullptr, model, &in, rule, commit, &wanted))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap);
    const size_t nz = size_t(ukfb::associate_out_scalars(candidates, e->cap, 3)), nk = size_t(ukfb::associate_out_scalars(candidates, e->cap, 1));
    ukfb::HostStage stage(e);
    in.model_dev = stage.raw_in(model_per_filter, n);
    in.z_dev = stage.in(z, nz);
    in.Q_dev = stage.in(Q, n * 9);
    in.mount_dev = stage.in(mount, n * 7);
    in.point_dev = stage.in(point, n * 3);
    ukfb_pda_out out{};
    out.z_pred = stage.out(z_pred, n * 3);
    out.S = stage.out(S, n * 9);
    out.innov = stage.out(innov, nz);
    out.maha = stage.out(maha, nk);
    out.loglik = stage.out(loglik, nk);
    out.beta = stage.out(beta, nk);
    out.beta0 = stage.out(beta0, n);
    out.innov_comb = stage.out(innov_comb, n * 3);
    out.best = stage.raw_out(best, n);
    out.n_gated = stage.raw_out(n_gated, n);
    out.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_update_pda_dev(e, model, &in, rule, commit, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
