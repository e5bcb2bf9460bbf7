// ukf_delayed_api.hip -- C-ABI of the delayed-measurement update (include/ukf_batch.h, "late samples"): argument checks
// (ukf_host.hpp), the device form, the lag helper and the host-array form.
#include <vector>

#include "ukf_api_common.hpp"
#include "ukf_delayed_req.hpp"

namespace ukfb {

// ukfb_delayed_lag_dev: one thread per filter, the window's stamps by value
struct DelayedLagArgs {
    int64_t n;
    int steps;
    const int64_t* sample_ts;
    int32_t* lag_out;
    int64_t step_ts[DELAYED_MAX_STEPS];
};
__global__ void delayed_lag_kernel(const DelayedLagArgs a) {
    const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i >= a.n) return;
    a.lag_out[i] = delayed_lag_of(a.steps, a.step_ts, a.sample_ts[i]);
}

}  // namespace ukfb

namespace {

int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return ukfb::refuse_poisoned(e);
}

}  // namespace

extern "C" {

int ukfb_update_delayed_dev(ukfb_engine* e, const ukfb_delayed_in* in, int commit, const ukfb_delayed_out* out) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_delayed_args(in, commit, out))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    ukfb::DelayedReq r;
    r.in = *in;   // (in->dt is copied into the kernel arguments: nothing of the caller's is read after the call returns)
    r.commit = commit != 0;
    if (out) r.out = *out;
    return e->model == UKFB_MODEL_POSE ? ukfb::launch_delayed_pose(e, r) : ukfb::launch_delayed_orient(e, r);
}

int ukfb_delayed_lag_dev(ukfb_engine* e, int steps, const int64_t* step_ts_us, const int64_t* sample_ts_us_dev, int32_t* lag_out_dev) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_delayed_lag_args(steps, step_ts_us, sample_ts_us_dev != nullptr, lag_out_dev != nullptr)))
        return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    if (e->cap == 0) return UKFB_OK;
    ukfb::DelayedLagArgs a{};
    a.n = e->cap;
    a.steps = steps;
    a.sample_ts = sample_ts_us_dev;
    a.lag_out = lag_out_dev;
    for (int c = 0; c < steps; ++c) a.step_ts[c] = step_ts_us[c];
    const unsigned grid = unsigned((e->cap + 255) / 256);
    hipLaunchKernelGGL(ukfb::delayed_lag_kernel, dim3(grid), dim3(256), 0, ukfb::main_stream(e), a);
    return ukfb::launch_status("delayed-lag kernel launch");
}

int ukfb_update_delayed(ukfb_engine* e, int steps, const double* dt, const double* mu_hist, const double* cov_hist, const double* in_a,
                        const double* in_b, int lag_uniform, const int32_t* lag, int meas_model, const int32_t* meas_model_per_filter,
                        const double* z, const double* Q, int commit, double* z_pred, double* S, double* innov, double* maha,
                        double* loglik, uint32_t* status, double* mu_out, double* cov_out) {
    if (const int rc = entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_delayed_in in{};
    in.steps = steps;
    in.dt = dt;
    in.slots = steps;
    in.first_slot = 0;
    in.mu_hist_dev = mu_hist;
    in.cov_hist_dev = cov_hist;
    in.lag_uniform = lag_uniform;
    in.meas_model_uniform = meas_model;
    in.z_dev = z;
    in.Q_dev = Q;
    ukfb_delayed_out wanted{z_pred, S, innov, maha, loglik, status, mu_out, cov_out};
    if (const int rc = ukfb::fail(ukfb::check_delayed_args(&in, commit, &wanted))) return rc;
    ukfb::DeviceScope scope(e->device);
    UKFB_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), ts = e->tsize, SS = size_t(e->S), PK = size_t(e->PK), recs = size_t(steps) * n;
    ukfb::DeviceBuffers buf;
    void *mu_d = nullptr, *cov_d = nullptr, *a_d = nullptr, *b_d = nullptr, *z_d = nullptr, *q_d = nullptr;
    void *zp_d = nullptr, *s_d = nullptr, *inn_d = nullptr, *maha_d = nullptr, *ll_d = nullptr, *mo_d = nullptr, *co_d = nullptr;
    int32_t *lag_d = nullptr, *model_d = nullptr;
    uint32_t* st_d = nullptr;
    UKFB_HIP_TRY(buf.take(&mu_d, recs * SS * ts));
    UKFB_HIP_TRY(buf.take(&cov_d, recs * PK * ts));
    if (in_a) UKFB_HIP_TRY(buf.take(&a_d, recs * 3 * ts));
    if (in_b) UKFB_HIP_TRY(buf.take(&b_d, recs * 3 * ts));
    UKFB_HIP_TRY(buf.take(&z_d, n * 3 * ts));
    UKFB_HIP_TRY(buf.take(&q_d, n * 9 * ts));
    if (lag) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&lag_d), n * sizeof(int32_t)));
    if (meas_model_per_filter) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&model_d), n * sizeof(int32_t)));
    if (z_pred) UKFB_HIP_TRY(buf.take(&zp_d, n * 4 * ts));
    if (S) UKFB_HIP_TRY(buf.take(&s_d, n * 9 * ts));
    if (innov) UKFB_HIP_TRY(buf.take(&inn_d, n * 3 * ts));
    if (maha) UKFB_HIP_TRY(buf.take(&maha_d, n * ts));
    if (loglik) UKFB_HIP_TRY(buf.take(&ll_d, n * ts));
    if (status) UKFB_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), n * sizeof(uint32_t)));
    if (mu_out) UKFB_HIP_TRY(buf.take(&mo_d, n * SS * ts));
    if (cov_out) UKFB_HIP_TRY(buf.take(&co_d, n * PK * ts));
    std::vector<double> packed(recs * PK);
    ukfb::pack_lower(cov_hist, recs, e->D, packed.data());
    if (const int rc = ukfb::upload_scalars(e, mu_d, mu_hist, recs * SS)) return rc;
    if (const int rc = ukfb::upload_scalars(e, cov_d, packed.data(), recs * PK)) return rc;
    if (in_a)
        if (const int rc = ukfb::upload_scalars(e, a_d, in_a, recs * 3)) return rc;
    if (in_b)
        if (const int rc = ukfb::upload_scalars(e, b_d, in_b, recs * 3)) return rc;
    if (const int rc = ukfb::upload_scalars(e, z_d, z, n * 3)) return rc;
    if (const int rc = ukfb::upload_scalars(e, q_d, Q, n * 9)) return rc;
    if (lag_d) UKFB_HIP_TRY(hipMemcpyAsync(lag_d, lag, n * sizeof(int32_t), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    if (model_d) UKFB_HIP_TRY(hipMemcpyAsync(model_d, meas_model_per_filter, n * sizeof(int32_t), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    in.mu_hist_dev = mu_d;
    in.cov_hist_dev = cov_d;
    in.in_a_dev = a_d;
    in.in_b_dev = b_d;
    in.lag_dev = lag_d;
    in.meas_model_dev = model_d;
    in.z_dev = z_d;
    in.Q_dev = q_d;
    const ukfb_delayed_out out{zp_d, s_d, inn_d, maha_d, ll_d, st_d, mo_d, co_d};
    if (const int rc = ukfb_update_delayed_dev(e, &in, commit, &out)) return rc;
    if (z_pred)
        if (const int rc = ukfb::download_scalars(e, zp_d, z_pred, n * 4)) return rc;
    if (S)
        if (const int rc = ukfb::download_scalars(e, s_d, S, n * 9)) return rc;
    if (innov)
        if (const int rc = ukfb::download_scalars(e, inn_d, innov, n * 3)) return rc;
    if (maha)
        if (const int rc = ukfb::download_scalars(e, maha_d, maha, n)) return rc;
    if (loglik)
        if (const int rc = ukfb::download_scalars(e, ll_d, loglik, n)) return rc;
    if (mu_out)
        if (const int rc = ukfb::download_scalars(e, mo_d, mu_out, n * SS)) return rc;
    if (cov_out) {
        std::vector<double> pk(n * PK);
        if (const int rc = ukfb::download_scalars(e, co_d, pk.data(), n * PK)) return rc;
        ukfb::unpack_symmetric(pk.data(), n, e->D, cov_out);
    }
    if (status) UKFB_HIP_TRY(hipMemcpyAsync(status, st_d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);   // (the temporaries are freed after the stream has drained)
}

}  // extern "C"
