// ukf_smooth_api.hip -- C-ABI of the fixed-interval smoother (include/ukf_batch.h, "fixed-interval smoothing"): argument
// checks and the chunking of a window into launches (ukf_host.hpp), the history push, and the host-array form.
#include <vector>

#include "ukf_smooth_req.hpp"

namespace {

int fail(const ukfb::Verdict& v) {
    if (v.rc != UKFB_OK) ukfb::set_error_text(v.msg ? v.msg : "invalid argument");
    return v.rc;
}

#define SMOOTH_HIP_TRY(expr)                       \
    do {                                           \
        const hipError_t _e = (expr);              \
        if (_e != hipSuccess) {                    \
            ukfb::set_error(#expr, _e);            \
            return UKFB_ERR_HIP;                   \
        }                                          \
    } while (0)

struct DeviceBuffers {   // temporaries of the host-array form, freed on every path
    std::vector<void*> ptrs;
    ~DeviceBuffers() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    hipError_t take(void** p, size_t bytes) {
        const hipError_t err = hipMalloc(p, bytes ? bytes : 1);
        if (err == hipSuccess) ptrs.push_back(*p);
        return err;
    }
};

int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (e->poisoned) return fail({UKFB_ERR_HIP, "engine poisoned by an earlier wait that timed out (UKFB_WAIT_TIMEOUT_S)"});
    return UKFB_OK;
}

// host doubles <-> engine precision on the device (through a host copy: the host-array form is a convenience, not a hot path)
int upload_scalars(ukfb_engine* e, void* dst, const double* src, size_t n) {
    if (e->prec == UKFB_F64) {
        SMOOTH_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, ukfb::main_stream(e)));
        return ukfb_sync(e);
    }
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = float(src[i]);
    SMOOTH_HIP_TRY(hipMemcpyAsync(dst, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    return ukfb_sync(e);
}

int download_scalars(ukfb_engine* e, const void* src, double* dst, size_t n) {
    if (e->prec == UKFB_F64) {
        SMOOTH_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
        return ukfb_sync(e);
    }
    std::vector<float> tmp(n);
    SMOOTH_HIP_TRY(hipMemcpyAsync(tmp.data(), src, n * sizeof(float), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    if (const int rc = ukfb_sync(e)) return rc;
    for (size_t i = 0; i < n; ++i) dst[i] = double(tmp[i]);
    return UKFB_OK;
}

// The chain's covariance between the launches of a window that has no covariance output: one record [capacity][PK], created
// the first time the engine records a history (or, for a caller that fills its rings itself, the first time such a window
// needs it) and kept.  Every smoother call of an engine is ordered on its stream, so one record serves all of them.
int ensure_chain_workspace(ukfb_engine* e) {
    if (e->smooth_chain) return UKFB_OK;
    const size_t bytes = size_t(e->cap) * size_t(e->PK) * e->tsize;
    SMOOTH_HIP_TRY(hipMalloc(&e->smooth_chain, bytes ? bytes : 1));
    return UKFB_OK;
}

}  // namespace

extern "C" {

int ukfb_history_push_dev(ukfb_engine* e, int slots, int slot, void* mu_hist_dev, void* cov_hist_dev) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = fail(ukfb::check_history_args(slots, slot, mu_hist_dev != nullptr, cov_hist_dev != nullptr))) return rc;
    ukfb::DeviceScope scope(e->device);
    SMOOTH_HIP_TRY(scope.err);
    const size_t mu_bytes = size_t(e->cap) * size_t(e->S) * e->tsize, cov_bytes = size_t(e->cap) * size_t(e->PK) * e->tsize;
    if (e->cap == 0) return UKFB_OK;
    if (const int rc = ensure_chain_workspace(e)) return rc;   // (the first push of an engine: ukfb_smooth_dev then never allocates)
    hipStream_t s = ukfb::main_stream(e);   // joins the second half of a split launch first
    SMOOTH_HIP_TRY(hipMemcpyAsync(static_cast<char*>(mu_hist_dev) + size_t(slot) * mu_bytes, e->mu, mu_bytes, hipMemcpyDeviceToDevice, s));
    SMOOTH_HIP_TRY(hipMemcpyAsync(static_cast<char*>(cov_hist_dev) + size_t(slot) * cov_bytes, e->cov, cov_bytes, hipMemcpyDeviceToDevice, s));
    return UKFB_OK;
}

int ukfb_smooth_dev(ukfb_engine* e, int steps, const double* dt, int slots, int first_slot, const void* mu_hist_dev,
                    const void* cov_hist_dev, const void* in_a_dev, const void* in_b_dev, void* mu_out_dev, void* cov_out_dev,
                    uint32_t* status_dev) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = fail(ukfb::check_smooth_args(steps, slots, first_slot, dt != nullptr, mu_hist_dev != nullptr,
                                                    cov_hist_dev != nullptr, mu_out_dev != nullptr)))
        return rc;
    ukfb::DeviceScope scope(e->device);
    SMOOTH_HIP_TRY(scope.err);
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
        const int rc = e->model == UKFB_MODEL_POSE ? ukfb::launch_smooth_pose(e, r) : ukfb::launch_smooth_orient(e, r);
        if (rc != UKFB_OK) return rc;
    }
    return UKFB_OK;
}

int ukfb_smooth(ukfb_engine* e, int steps, const double* dt, double* mu, double* cov, const double* in_a, const double* in_b,
                uint32_t* status) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = fail(ukfb::check_smooth_args(steps, steps, 0, dt != nullptr, mu != nullptr, cov != nullptr, mu != nullptr))) return rc;
    ukfb::DeviceScope scope(e->device);
    SMOOTH_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), ts = e->tsize, S = size_t(e->S), D = size_t(e->D), PK = size_t(e->PK), recs = size_t(steps) * n;
    DeviceBuffers buf;
    void *mu_d = nullptr, *cov_d = nullptr, *a_d = nullptr, *b_d = nullptr;
    uint32_t* st_d = nullptr;
    SMOOTH_HIP_TRY(buf.take(&mu_d, recs * S * ts));
    SMOOTH_HIP_TRY(buf.take(&cov_d, recs * PK * ts));
    if (in_a) SMOOTH_HIP_TRY(buf.take(&a_d, recs * 3 * ts));
    if (in_b) SMOOTH_HIP_TRY(buf.take(&b_d, recs * 3 * ts));
    if (status) SMOOTH_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), n * sizeof(uint32_t)));
    std::vector<double> packed(recs * PK);
    for (size_t i = 0; i < recs; ++i)
        for (size_t r = 0; r < D; ++r)
            for (size_t c = 0; c <= r; ++c) packed[i * PK + r * (r + 1) / 2 + c] = cov[(i * D + r) * D + c];
    if (const int rc = upload_scalars(e, mu_d, mu, recs * S)) return rc;
    if (const int rc = upload_scalars(e, cov_d, packed.data(), recs * PK)) return rc;
    if (in_a)
        if (const int rc = upload_scalars(e, a_d, in_a, recs * 3)) return rc;
    if (in_b)
        if (const int rc = upload_scalars(e, b_d, in_b, recs * 3)) return rc;
    if (const int rc = ukfb_smooth_dev(e, steps, dt, steps, 0, mu_d, cov_d, a_d, b_d, mu_d, cov_d, st_d)) return rc;   // in place
    if (const int rc = download_scalars(e, mu_d, mu, recs * S)) return rc;
    if (const int rc = download_scalars(e, cov_d, packed.data(), recs * PK)) return rc;
    for (size_t i = 0; i < recs; ++i)
        for (size_t r = 0; r < D; ++r)
            for (size_t c = 0; c <= r; ++c) {
                const double v = packed[i * PK + r * (r + 1) / 2 + c];
                cov[(i * D + r) * D + c] = v;
                cov[(i * D + c) * D + r] = v;
            }
    if (status) SMOOTH_HIP_TRY(hipMemcpyAsync(status, st_d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);   // (the temporaries are freed after the stream has drained)
}

}  // extern "C"
