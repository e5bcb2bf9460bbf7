// ukf_runtime.hip -- the definitions behind ukf_api_common.hpp: the thread-local error channel (ukfb_last_error), the bounded
// waits on HIP streams and events, ukfb_sync, the transfers between host doubles and the engine's arrays with their conversion
// kernels, and launch, the dispatch of a launch request to the (precision, model) translation unit.
#include <cstdlib>
#include <string>
#include <vector>

#include "ukf_api_common.hpp"

namespace {
thread_local std::string g_last_error;

// pack / convert host doubles into engine precision -------------------------------------------
template <class T> void convert(const double* src, T* dst, size_t n) {
    for (size_t i = 0; i < n; ++i) dst[i] = T(src[i]);
}

__global__ void narrow_kernel(const double* src, float* dst, size_t n) {
    const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
    if (i < n) dst[i] = float(src[i]);
}
__global__ void widen_kernel(const float* src, double* dst, size_t n) {
    const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
    if (i < n) dst[i] = double(src[i]);
}

double wait_timeout_seconds() {
    static const double t = ukfb::wait_timeout_seconds(std::getenv("UKFB_WAIT_TIMEOUT_S"));
    return t;
}

// A bounded wait that gave up wrote its text and POISONED the engine: work of unknown state is still queued (see ENGINE_SYNC)
template <class Query> int bounded_wait(ukfb_engine* e, const char* what, Query&& query) {
    const ukfb::Waited<hipError_t> w = ukfb::wait_polling(query, hipErrorNotReady, ukfb::WAIT_SPINS, wait_timeout_seconds());
    if (w.gave_up) {
        e->poisoned = true;
        g_last_error = "timed out waiting for the engine's stream (UKFB_WAIT_TIMEOUT_S)";
        return UKFB_ERR_HIP;
    }
    if (w.result == hipSuccess) return UKFB_OK;
    ukfb::set_error(what, w.result);
    return UKFB_ERR_HIP;
}
}  // namespace

namespace ukfb {
void set_error(const char* what, hipError_t err) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(err);
}
void set_error_text(const std::string& text) { g_last_error = text; }

int wait_stream(ukfb_engine* e, hipStream_t s, const char* what) {
    return bounded_wait(e, what, [s] { return hipStreamQuery(s); });
}
int wait_event(ukfb_engine* e, hipEvent_t ev, const char* what) {
    return bounded_wait(e, what, [ev] { return hipEventQuery(ev); });
}

int engine_wait(ukfb_engine* e) {
    if (const int rc = refuse_poisoned(e)) return rc;
    return wait_stream(e, ukfb::main_stream(e), "waiting for the engine's stream");
}

bool range_ok(const ukfb_engine* e, int64_t first, int64_t count) {
    return e && first >= 0 && count >= 0 && first + count <= e->cap;
}

int check_meas_model(const ukfb_engine* e, int m) {
    return ukfb::meas_model_ok(e->model, m) ? UKFB_OK : fail(UKFB_ERR_WRONG_MODEL, "measurement model id not valid for this engine");
}

int upload(ukfb_engine* e, void* dst_dev, size_t elem_offset, const double* src, size_t n) {
    if (n == 0) return UKFB_OK;
    if (e->prec == UKFB_F64) {
        HIP_TRY(hipMemcpyAsync(static_cast<double*>(dst_dev) + elem_offset, src, n * sizeof(double),
                               hipMemcpyHostToDevice, ukfb::main_stream(e)));
        ENGINE_SYNC(e);
    } else if (n < DEVICE_CONVERT_MIN) {
        std::vector<float> tmp(n);
        convert(src, tmp.data(), n);
        HIP_TRY(hipMemcpyAsync(static_cast<float*>(dst_dev) + elem_offset, tmp.data(), n * sizeof(float),
                               hipMemcpyHostToDevice, ukfb::main_stream(e)));
        ENGINE_SYNC(e);
    } else {
        // fp32 engine, large array: the doubles cross PCIe as they are and are narrowed on the device (a
        // single-threaded host loop over 12 M values per cycle took ten times longer than the copy)
        {
            const int rc = ensure_scratch(e, n * sizeof(double));
            if (rc) return rc;
        }
        HIP_TRY(hipMemcpyAsync(e->cvt_dev, src, n * sizeof(double), hipMemcpyHostToDevice, ukfb::main_stream(e)));
        hipLaunchKernelGGL(narrow_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, ukfb::main_stream(e),
                           static_cast<const double*>(e->cvt_dev), static_cast<float*>(dst_dev) + elem_offset, n);
        HIP_TRY(hipGetLastError());
        ENGINE_SYNC(e);
    }
    return UKFB_OK;
}

// grow-only device scratch (see ukfb_engine::cvt_dev)
int ensure_scratch(ukfb_engine* e, size_t bytes) {
    if (e->cvt_bytes >= bytes) return UKFB_OK;
    ENGINE_SYNC(e);
    if (e->cvt_dev) HIP_TRY(hipFree(e->cvt_dev));
    e->cvt_dev = nullptr;
    e->cvt_bytes = 0;
    HIP_TRY(hipMalloc(&e->cvt_dev, bytes));
    e->cvt_bytes = bytes;
    return UKFB_OK;
}

int download(ukfb_engine* e, const void* src_dev, size_t elem_offset, double* dst, size_t n) {
    if (n == 0) return UKFB_OK;
    if (e->prec == UKFB_F64) {
        HIP_TRY(hipMemcpyAsync(dst, static_cast<const double*>(src_dev) + elem_offset, n * sizeof(double),
                               hipMemcpyDeviceToHost, ukfb::main_stream(e)));
        ENGINE_SYNC(e);
    } else if (n < DEVICE_CONVERT_MIN) {
        std::vector<float> tmp(n);
        HIP_TRY(hipMemcpyAsync(tmp.data(), static_cast<const float*>(src_dev) + elem_offset, n * sizeof(float),
                               hipMemcpyDeviceToHost, ukfb::main_stream(e)));
        ENGINE_SYNC(e);
        for (size_t i = 0; i < n; ++i) dst[i] = double(tmp[i]);
    } else {   // fp32 engine, large array: widened on the device, the doubles cross PCIe as they are
        int rc = ensure_scratch(e, n * sizeof(double));
        if (rc) return rc;
        hipLaunchKernelGGL(widen_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, ukfb::main_stream(e),
                           static_cast<const float*>(src_dev) + elem_offset, static_cast<double*>(e->cvt_dev), n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(dst, e->cvt_dev, n * sizeof(double), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
        ENGINE_SYNC(e);
    }
    return UKFB_OK;
}

// host doubles -> device array in engine precision, enqueued on the copy stream (no wait)
int upload_on_copy_stream(ukfb_engine* e, void* dst_dev, const double* src, size_t n) {
    if (n == 0) return UKFB_OK;
    if (e->prec == UKFB_F64) {
        HIP_TRY(hipMemcpyAsync(dst_dev, src, n * sizeof(double), hipMemcpyHostToDevice, e->copy_stream));
        return UKFB_OK;
    }
    // fp32: the doubles cross PCIe as they are and are narrowed on the device (cf. upload)
    HIP_TRY(hipMemcpyAsync(e->cvt_copy, src, n * sizeof(double), hipMemcpyHostToDevice, e->copy_stream));
    hipLaunchKernelGGL(narrow_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, e->copy_stream,
                       static_cast<const double*>(e->cvt_copy), static_cast<float*>(dst_dev), n);
    HIP_TRY(hipGetLastError());
    return UKFB_OK;
}

int fill_scalar(ukfb_engine* e, void* dst_dev, size_t n, double value) {
    std::vector<double> v(n, value);
    return upload(e, dst_dev, 0, v.data(), n);
}

int launch(ukfb_engine* e, const ukfb::LaunchReq& r) {
    if (const int rc = refuse_poisoned(e)) return rc;
    ON_DEVICE(e->device);
    if (r.wait_event) HIP_TRY(hipStreamWaitEvent(ukfb::main_stream(e), r.wait_event, 0));
    int rc;
    const bool wide = e->prec == UKFB_F32 && e->cfg.wide_arithmetic != 0;   // fp32 arrays, fp64 arithmetic (tuned layout only)
    if (e->model == UKFB_MODEL_POSE)
        rc = e->prec == UKFB_F64 ? ukfb::launch_pose_f64(e, r) : (wide ? ukfb::launch_pose_f32w(e, r) : ukfb::launch_pose_f32(e, r));
    else
        rc = e->prec == UKFB_F64 ? ukfb::launch_orient_f64(e, r) : (wide ? ukfb::launch_orient_f32w(e, r) : ukfb::launch_orient_f32(e, r));
    if (!rc && r.done_event) HIP_TRY(hipEventRecord(r.done_event, ukfb::main_stream(e)));
    return rc;
}
}  // namespace ukfb

extern "C" {

const char* ukfb_last_error(void) { return g_last_error.c_str(); }

int ukfb_sync(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return ukfb::engine_wait(e);
}

}  // extern "C"
