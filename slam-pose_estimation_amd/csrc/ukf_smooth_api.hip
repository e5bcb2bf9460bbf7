// ukf_smooth_api.hip -- C-ABI of the fixed-interval smoother (include/ukf_batch.h, "fixed-interval smoothing"): argument
// checks and the chunking of a window into launches (ukf_host.hpp), the history push, and the host-array form.
#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

namespace {

// The chain's covariance between the launches of a window that has no covariance output: one record [capacity][PK], created
// the first time the engine records a history (or, for a caller that fills its rings itself, the first time such a window
// needs it) and kept.  Every smoother call of an engine is ordered on its stream, so one record serves all of them.
int ensure_chain_workspace(ukfb_engine* e) {
    if (e->smooth_chain) return UKFB_OK;
    const size_t bytes = size_t(e->cap) * size_t(e->PK) * e->tsize;
    HIP_TRY(hipMalloc(&e->smooth_chain, bytes ? bytes : 1));
    return UKFB_OK;
}

}  // namespace

extern "C" {

int ukfb_history_push_dev(ukfb_engine* e, int slots, int slot, void* mu_hist_dev, void* cov_hist_dev) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_history_args(slots, slot, mu_hist_dev != nullptr, cov_hist_dev != nullptr))) return rc;
    ON_DEVICE(e->device);
    const size_t mu_bytes = size_t(e->cap) * size_t(e->S) * e->tsize, cov_bytes = size_t(e->cap) * size_t(e->PK) * e->tsize;
    if (e->cap == 0) return UKFB_OK;
    if (const int rc = ensure_chain_workspace(e)) return rc;   // (the first push of an engine: ukfb_smooth_dev then never allocates)
    hipStream_t s = ukfb::main_stream(e);   // joins the second half of a split launch first
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(mu_hist_dev) + size_t(slot) * mu_bytes, e->mu, mu_bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(cov_hist_dev) + size_t(slot) * cov_bytes, e->cov, cov_bytes, hipMemcpyDeviceToDevice, s));
    return UKFB_OK;
}

int ukfb_smooth_dev(ukfb_engine* e, int steps, const double* dt, int slots, int first_slot, const void* mu_hist_dev,
                    const void* cov_hist_dev, const void* in_a_dev, const void* in_b_dev, void* mu_out_dev, void* cov_out_dev,
                    uint32_t* status_dev) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_smooth_args(steps, slots, first_slot, dt != nullptr, mu_hist_dev != nullptr,
                                                          cov_hist_dev != nullptr, mu_out_dev != nullptr)))
        return rc;
    ON_DEVICE(e->device);
    const ukfb::SmoothPlan plan(steps, slots, first_slot);
    const size_t cov_rec = size_t(e->cap) * size_t(e->PK) * e->tsize;
    // without a covariance output the chain's covariance crosses a launch boundary through the engine's workspace
    if (!cov_out_dev && plan.launches() > 1)
        if (const int rc = ensure_chain_workspace(e)) return rc;
    ukfb::SmoothReq r;
    r.slots = slots;
    r.dt = dt;   // copied into the kernel arguments: nothing of the caller's is read after the call returns
    r.mu_hist_dev = mu_hist_dev;
    r.cov_hist_dev = cov_hist_dev;
    r.in_a_dev = in_a_dev;
    r.in_b_dev = in_b_dev;
    r.mu_out_dev = mu_out_dev;
    r.cov_out_dev = cov_out_dev;
    r.status_dev = status_dev;
    for (int k = 0; k < plan.launches(); ++k) {
        r.part = plan[k];
        r.start_cov_dev = cov_out_dev ? static_cast<const void*>(static_cast<char*>(cov_out_dev) + size_t(r.part.top_slot) * cov_rec)
                                      : static_cast<const void*>(e->smooth_chain);
        r.end_cov_dev = (!cov_out_dev && k + 1 < plan.launches()) ? e->smooth_chain : nullptr;
        const int rc = ukfb::launch_for_model(e, r);
        if (rc != UKFB_OK) return rc;
    }
    return UKFB_OK;
}

int ukfb_smooth(ukfb_engine* e, int steps, const double* dt, double* mu, double* cov, const double* in_a, const double* in_b,
                uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_smooth_args(steps, steps, 0, dt != nullptr, mu != nullptr, cov != nullptr, mu != nullptr))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), recs = size_t(steps) * n;
    ukfb::HostStage stage(e);
    void* mu_d = stage.inout(mu, recs * size_t(e->S));
    void* cov_d = stage.cov_inout(cov, recs);
    const void* a_d = stage.in(in_a, recs * 3);
    const void* b_d = stage.in(in_b, recs * 3);
    uint32_t* st_d = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_smooth_dev(e, steps, dt, steps, 0, mu_d, cov_d, a_d, b_d, mu_d, cov_d, st_d)) return rc;   // in place
    return stage.finish();
}

}  // extern "C"
