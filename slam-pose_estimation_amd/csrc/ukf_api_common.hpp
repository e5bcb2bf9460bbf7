// ukf_api_common.hpp -- the host plumbing the feature C-ABI files share (every ukf_*_api.hip: the Makefile's FEATURES): the
// error macro, the argument verdict, the poisoned-engine refusal and the temporaries and copies of the host-array forms.  Not for ukf_batch.hip / ukf_group.hip: their HIP_TRY knows the timed-out
// wait and their fail has another signature.
#pragma once

#include <vector>

#include "ukf_engine.hpp"

#define UKFB_HIP_TRY(expr)                         \
    do {                                           \
        const hipError_t _e = (expr);              \
        if (_e != hipSuccess) {                    \
            ukfb::set_error(#expr, _e);            \
            return UKFB_ERR_HIP;                   \
        }                                          \
    } while (0)

namespace ukfb {

inline int fail(const ukfb::Verdict& v) {
    if (v.rc != UKFB_OK) set_error_text(v.msg ? v.msg : "invalid argument");
    return v.rc;
}

// UKFB_OK, or the refusal of an engine one of whose bounded waits gave up (every entry point decides where it asks)
inline int refuse_poisoned(const ukfb_engine* e) {
    if (e->poisoned) return fail({UKFB_ERR_HIP, "engine poisoned by an earlier wait that timed out (UKFB_WAIT_TIMEOUT_S)"});
    return UKFB_OK;
}

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

// host doubles <-> engine precision on the device (through a host copy: the host-array forms are a convenience, not a hot path)
inline int upload_scalars(ukfb_engine* e, void* dst, const double* src, size_t n) {
    if (e->prec == UKFB_F64) {
        UKFB_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, ukfb::main_stream(e)));
        return ukfb_sync(e);
    }
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = float(src[i]);
    UKFB_HIP_TRY(hipMemcpyAsync(dst, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    return ukfb_sync(e);
}

inline int download_scalars(ukfb_engine* e, const void* src, double* dst, size_t n) {
    if (e->prec == UKFB_F64) {
        UKFB_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
        return ukfb_sync(e);
    }
    std::vector<float> tmp(n);
    UKFB_HIP_TRY(hipMemcpyAsync(tmp.data(), src, n * sizeof(float), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    if (const int rc = ukfb_sync(e)) return rc;
    for (size_t i = 0; i < n; ++i) dst[i] = double(tmp[i]);
    return UKFB_OK;
}

}  // namespace ukfb
