// ukf_state_meas_api.hip -- C-ABI of the joint state-block measurements (include/ukf_batch.h, "joint state-block
// measurements"): argument checks (ukf_host.hpp), the device form, the host-array form and the RigidBodyState adapter.
#include <vector>

#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

extern "C" {

int ukfb_update_state_dev(ukfb_engine* e, uint32_t block_mask_uniform, const int32_t* block_mask_dev, const void* z_dev,
                          const void* Qz_packed_dev, double state_inflation, double meas_inflation, int commit,
                          const ukfb_state_meas_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_state_meas_args(e->model, block_mask_dev != nullptr, block_mask_uniform, z_dev != nullptr,
                                                              Qz_packed_dev != nullptr, state_inflation, meas_inflation, commit, out)))
        return rc;
    ON_DEVICE(e->device);
    ukfb::StateMeasReq r;
    r.mask_uniform = block_mask_uniform;
    r.mask_dev = block_mask_dev;
    r.z_dev = z_dev;
    r.Qz_dev = Qz_packed_dev;
    r.state_inflation = state_inflation;
    r.meas_inflation = meas_inflation;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return ukfb::launch_for_model(e, r);
}

int ukfb_update_state(ukfb_engine* e, uint32_t block_mask, const int32_t* block_mask_per_filter, const double* z, const double* Qz,
                      double state_inflation, double meas_inflation, int commit, double* maha, double* loglik, uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (the outputs the device call will see: a buffer for each one the caller wants)
    ukfb_state_meas_out wanted{maha, loglik, status};
    if (const int rc = ukfb::fail(ukfb::check_state_meas_args(e->model, block_mask_per_filter != nullptr, block_mask, z != nullptr,
                                                              Qz != nullptr, state_inflation, meas_inflation, commit, &wanted)))
        return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap);
    ukfb::HostStage stage(e);
    const int32_t* mask_d = stage.raw_in(block_mask_per_filter, n);
    const void* z_d = stage.in(z, n * size_t(e->S));
    const void* q_d = stage.cov_in(Qz, n);
    ukfb_state_meas_out out{};
    out.maha = stage.out(maha, n);
    out.loglik = stage.out(loglik, n);
    out.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_update_state_dev(e, block_mask, mask_d, z_d, q_d, state_inflation, meas_inflation, commit, &out)) return rc;
    return stage.finish();
}

int ukfb_pose_update_body_states(ukfb_engine* e, uint32_t block_mask, const double* records, const uint8_t* active) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (e->model != UKFB_MODEL_POSE) return ukfb::fail({UKFB_ERR_WRONG_MODEL, "Pose engines only"});
    if (!records) return ukfb::fail({UKFB_ERR_INVALID_ARG, "records must not be NULL"});
    if (!ukfb::state_meas_mask_ok(ukfb::state_meas_blocks(e->model), int64_t(block_mask)))
        return ukfb::fail({UKFB_ERR_INVALID_ARG, "block_mask must select at least one block and none beyond the model's (Pose: 4, OrientationState: 5)"});
    const size_t n = size_t(e->cap);
    std::vector<double> z(n * 13), Qz(n * 144);
    for (size_t i = 0; i < n; ++i) ukfb::body_state_to_measurement(records + i * UKFB_BODY_STATE_SCALARS, z.data() + i * 13, Qz.data() + i * 144);
    std::vector<int32_t> masks;
    if (active) {
        masks.resize(n);
        for (size_t i = 0; i < n; ++i) masks[i] = active[i] ? int32_t(block_mask) : 0;
    }
    return ukfb_update_state(e, block_mask, active ? masks.data() : nullptr, z.data(), Qz.data(), 1.0, 1.0, 1, nullptr, nullptr, nullptr);
}

}  // extern "C"
