// ukf_bank_api.hip -- C-ABI of the filter banks (include/ukf_batch.h, "filter banks"): argument checks (ukf_host.hpp), the
// launch requests, and the host-array forms.
#include <cmath>
#include <vector>

#include "ukf_bank_req.hpp"

namespace {

int fail(const ukfb::Verdict& v) {
    if (v.rc != UKFB_OK) ukfb::set_error_text(v.msg ? v.msg : "invalid argument");
    return v.rc;
}

#define BANK_HIP_TRY(expr)                         \
    do {                                           \
        const hipError_t _e = (expr);              \
        if (_e != hipSuccess) {                    \
            ukfb::set_error(#expr, _e);            \
            return UKFB_ERR_HIP;                   \
        }                                          \
    } while (0)

struct DeviceBuffers {   // temporaries of the host-array forms, freed on every path
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

// host doubles <-> engine precision on the device (through a host copy: these forms are a convenience, not a hot path)
int upload_scalars(ukfb_engine* e, void* dst, const double* src, size_t n) {
    if (e->prec == UKFB_F64) {
        BANK_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, ukfb::main_stream(e)));
        return ukfb_sync(e);
    }
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = float(src[i]);
    BANK_HIP_TRY(hipMemcpyAsync(dst, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    return ukfb_sync(e);
}

int download_scalars(ukfb_engine* e, const void* src, double* dst, size_t n) {
    if (e->prec == UKFB_F64) {
        BANK_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
        return ukfb_sync(e);
    }
    std::vector<float> tmp(n);
    BANK_HIP_TRY(hipMemcpyAsync(tmp.data(), src, n * sizeof(float), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    if (const int rc = ukfb_sync(e)) return rc;
    for (size_t i = 0; i < n; ++i) dst[i] = double(tmp[i]);
    return UKFB_OK;
}

int entry(ukfb_engine* e, int hypotheses) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (const int rc = fail(ukfb::check_bank_args(hypotheses, e->cap))) return rc;
    if (e->poisoned) return fail({UKFB_ERR_HIP, "engine poisoned by an earlier wait that timed out (UKFB_WAIT_TIMEOUT_S)"});
    return UKFB_OK;
}

int launch(ukfb_engine* e, const ukfb::BankReq& r) {
    return e->model == UKFB_MODEL_POSE ? ukfb::launch_bank_pose(e, r) : ukfb::launch_bank_orient(e, r);
}

}  // namespace

extern "C" {

int ukfb_bank_weights_dev(ukfb_engine* e, int hypotheses, const void* logw_in_dev, const void* loglik_dev, void* logw_out_dev,
                          void* w_out_dev, uint32_t* status_dev) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!logw_out_dev) return fail({UKFB_ERR_INVALID_ARG, "logw_out must not be NULL"});
    ukfb::DeviceScope scope(e->device);
    BANK_HIP_TRY(scope.err);
    ukfb::BankWeightsReq r;
    r.hypotheses = hypotheses;
    r.logw_in_dev = logw_in_dev;
    r.loglik_dev = loglik_dev;
    r.logw_out_dev = logw_out_dev;
    r.w_out_dev = w_out_dev;
    r.status_dev = status_dev;
    return ukfb::launch_bank_weights(e, r);
}

int ukfb_bank_combine_dev(ukfb_engine* e, int hypotheses, const void* w_dev, void* mu_out_dev, void* cov_packed_out_dev,
                          uint32_t* status_dev) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!w_dev || !mu_out_dev) return fail({UKFB_ERR_INVALID_ARG, "w and mu_out must not be NULL"});
    ukfb::DeviceScope scope(e->device);
    BANK_HIP_TRY(scope.err);
    ukfb::BankReq r;
    r.hypotheses = hypotheses;
    r.w_dev = w_dev;
    r.mu_out_dev = mu_out_dev;
    r.cov_out_dev = cov_packed_out_dev;
    r.status_dev = status_dev;
    return launch(e, r);
}

int ukfb_bank_mix_dev(ukfb_engine* e, int hypotheses, const void* w_dev, const double* transition, void* w_pred_out_dev,
                      uint32_t* status_dev) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!w_dev || !w_pred_out_dev) return fail({UKFB_ERR_INVALID_ARG, "w and w_pred_out must not be NULL"});
    if (const int rc = fail(ukfb::check_bank_transition(transition, hypotheses))) return rc;
    ukfb::DeviceScope scope(e->device);
    BANK_HIP_TRY(scope.err);
    ukfb::BankReq r;
    r.hypotheses = hypotheses;
    r.mix = true;
    r.w_dev = w_dev;
    r.w_pred_dev = w_pred_out_dev;
    r.transition = transition;   // copied into the kernel arguments: nothing of the caller's is read after the call returns
    r.status_dev = status_dev;
    return launch(e, r);
}

int ukfb_bank_combine(ukfb_engine* e, int hypotheses, const double* w, double* mu, double* cov, uint32_t* status) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!w || !mu) return fail({UKFB_ERR_INVALID_ARG, "w and mu must not be NULL"});
    ukfb::DeviceScope scope(e->device);
    BANK_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), tracks = n / size_t(hypotheses), ts = e->tsize, S = size_t(e->S), D = size_t(e->D), PK = size_t(e->PK);
    DeviceBuffers buf;
    void *w_d = nullptr, *mu_d = nullptr, *cov_d = nullptr;
    uint32_t* st_d = nullptr;
    BANK_HIP_TRY(buf.take(&w_d, n * ts));
    BANK_HIP_TRY(buf.take(&mu_d, tracks * S * ts));
    if (cov) BANK_HIP_TRY(buf.take(&cov_d, tracks * PK * ts));
    if (status) BANK_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), tracks * sizeof(uint32_t)));
    if (const int rc = upload_scalars(e, w_d, w, n)) return rc;
    if (const int rc = ukfb_bank_combine_dev(e, hypotheses, w_d, mu_d, cov_d, st_d)) return rc;
    if (const int rc = download_scalars(e, mu_d, mu, tracks * S)) return rc;
    if (cov) {
        std::vector<double> packed(tracks * PK);
        if (const int rc = download_scalars(e, cov_d, packed.data(), tracks * PK)) return rc;
        for (size_t t = 0; t < tracks; ++t)
            for (size_t r = 0; r < D; ++r)
                for (size_t c = 0; c <= r; ++c) {
                    const double v = packed[t * PK + r * (r + 1) / 2 + c];
                    cov[(t * D + r) * D + c] = v;
                    cov[(t * D + c) * D + r] = v;
                }
    }
    if (status) BANK_HIP_TRY(hipMemcpyAsync(status, st_d, tracks * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);   // (the temporaries are freed after the stream has drained)
}

int ukfb_bank_mix(ukfb_engine* e, int hypotheses, const double* w, const double* transition, double* w_pred, uint32_t* status) {
    if (const int rc = entry(e, hypotheses)) return rc;
    if (!w || !w_pred) return fail({UKFB_ERR_INVALID_ARG, "w and w_pred must not be NULL"});
    if (const int rc = fail(ukfb::check_bank_transition(transition, hypotheses))) return rc;
    ukfb::DeviceScope scope(e->device);
    BANK_HIP_TRY(scope.err);
    const size_t n = size_t(e->cap), tracks = n / size_t(hypotheses), ts = e->tsize;
    DeviceBuffers buf;
    void *w_d = nullptr, *wp_d = nullptr;
    uint32_t* st_d = nullptr;
    BANK_HIP_TRY(buf.take(&w_d, n * ts));
    BANK_HIP_TRY(buf.take(&wp_d, n * ts));
    if (status) BANK_HIP_TRY(buf.take(reinterpret_cast<void**>(&st_d), tracks * sizeof(uint32_t)));
    if (const int rc = upload_scalars(e, w_d, w, n)) return rc;
    if (const int rc = ukfb_bank_mix_dev(e, hypotheses, w_d, transition, wp_d, st_d)) return rc;
    if (const int rc = download_scalars(e, wp_d, w_pred, n)) return rc;
    if (status) BANK_HIP_TRY(hipMemcpyAsync(status, st_d, tracks * sizeof(uint32_t), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    return ukfb_sync(e);
}

}  // extern "C"
