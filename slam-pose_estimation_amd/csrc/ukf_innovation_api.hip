// ukf_innovation_api.hip -- C-ABI of the read-only innovation statistics (include/ukf_batch.h, "innovation statistics and
// measurement association"): argument checks (ukf_host.hpp), the launch requests, and the host-array form.
#include "ukf_api_common.hpp"
#include "ukf_innovation.hpp"
#include "ukf_feature_req.hpp"

extern "C" {

int ukfb_innovation_dev(ukfb_engine* e, int meas_model_uniform, const int32_t* meas_model_dev, int candidates, const void* z_dev,
                        const void* Q_dev, int q_is_uniform, const ukfb_innovation_out* out) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (const int rc = ukfb::fail(ukfb::check_innovation_args(e->model, meas_model_dev != nullptr, meas_model_uniform, candidates,
                                                              z_dev != nullptr, Q_dev != nullptr, out)))
        return rc;
    if (const int rc = ukfb::refuse_poisoned(e)) return rc;
    ON_DEVICE(e->device);
    ukfb::InnovReq r;
    r.meas_uniform = meas_model_uniform;
    r.meas_dev = meas_model_dev;
    r.candidates = candidates;
    r.z_dev = z_dev;
    r.Q_dev = Q_dev;
    r.q_uniform = q_is_uniform != 0;
    r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_select_candidates_dev(ukfb_engine* e, int candidates, const int32_t* best_dev, int meas_model_uniform,
                               const int32_t* meas_model_dev, const void* z_dev, void* z_sel_dev, int32_t* meas_model_sel_dev) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (const int rc = ukfb::fail(ukfb::check_select_args(e->model, meas_model_dev != nullptr, meas_model_uniform, candidates,
                                                          best_dev != nullptr, z_dev != nullptr, z_sel_dev != nullptr)))
        return rc;
    if (const int rc = ukfb::refuse_poisoned(e)) return rc;
    ON_DEVICE(e->device);
    if (e->cap == 0) return UKFB_OK;
    const dim3 gd((unsigned)((e->cap + 255) / 256)), bd(256);
    if (e->prec == UKFB_F64)
        hipLaunchKernelGGL(ukfb::select_candidates_kernel<double>, gd, bd, 0, ukfb::main_stream(e), e->cap, candidates, best_dev,
                           meas_model_uniform, meas_model_dev, static_cast<const double*>(z_dev), static_cast<double*>(z_sel_dev),
                           meas_model_sel_dev);
    else
        hipLaunchKernelGGL(ukfb::select_candidates_kernel<float>, gd, bd, 0, ukfb::main_stream(e), e->cap, candidates, best_dev,
                           meas_model_uniform, meas_model_dev, static_cast<const float*>(z_dev), static_cast<float*>(z_sel_dev),
                           meas_model_sel_dev);
    HIP_TRY(hipGetLastError());
    return UKFB_OK;
}

int ukfb_innovation(ukfb_engine* e, int meas_model, int candidates, const double* z, const double* Q, double* z_pred, double* S,
                    double* innov, double* maha, double* loglik, int32_t* best, uint32_t* status) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    ukfb_innovation_out asked{};   // non-NULL where the caller wants the output (checked before anything is allocated)
    asked.z_pred = z_pred; asked.S = S; asked.innov = innov; asked.maha = maha; asked.loglik = loglik;
    asked.best = best; asked.status = status;
    if (const int rc = ukfb::fail(ukfb::check_innovation_args(e->model, false, meas_model, candidates, z != nullptr, Q != nullptr, &asked)))
        return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), K = size_t(candidates);
    ukfb::HostStage stage(e);
    const void* z_d = stage.in(z, K * n * 3);
    const void* Q_d = stage.in(Q, n * 9);
    ukfb_innovation_out o{};
    o.z_pred = stage.out(z_pred, n * 4);
    o.S = stage.out(S, n * 9);
    o.innov = stage.out(innov, K * n * 3);
    o.maha = stage.out(maha, K * n);
    o.loglik = stage.out(loglik, K * n);
    o.best = stage.raw_out(best, n);
    o.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_innovation_dev(e, meas_model, nullptr, candidates, z_d, Q_d, 0, &o)) return rc;
    return stage.finish();
}

}  // extern "C"
