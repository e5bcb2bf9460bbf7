// ukf_api_common.hpp -- the host plumbing every host translation unit shares (the Makefile's HOST_TUS and every ukf_*_api.hip):
// the error macro and the device scope, the argument verdict, the entry check with the poisoned-engine refusal, the owner of a
// temporary device buffer, the bounded waits, the transfers between host doubles and the engine's arrays, and HostStage, the
// one place where the host-array forms allocate their temporaries and copy to and from the device.  What is only declared
// here is defined once, in namespace ukfb: the error channel, the waits, the transfers and launch in ukf_runtime.hip,
// build_model_buckets in ukf_buckets.hip, rebuild_racc in ukf_batch.hip, launch_assign in ukf_assign_launch.hip, launch_jpda in ukf_jpda_launch.hip.
#pragma once

#include <algorithm>
#include <vector>

#include "ukf_engine.hpp"

#define HIP_TRY(expr)                              \
    do {                                           \
        const hipError_t _e = (expr);              \
        if (_e != hipSuccess) {                    \
            ukfb::set_error(#expr, _e);            \
            return UKFB_ERR_HIP;                   \
        }                                          \
    } while (0)

// the engine's device for the rest of the enclosing scope, the caller's device again afterwards (ukfb::DeviceScope)
#define ON_DEVICE(dev)                                     \
    ukfb::DeviceScope device_scope_(dev);                  \
    HIP_TRY(device_scope_.err)

// Waits for the engine's stream with the bounded polling wait (ukfb::engine_wait).  A wait that gives up POISONS the engine:
// work of unknown state is still queued, so every later call fails fast with UKFB_ERR_HIP, and ukfb_destroy neither waits
// again nor frees device memory that a kernel in flight may still touch (the process is expected to exit non-zero).
#define ENGINE_SYNC(e)                                     \
    do {                                                   \
        const int _rc = ukfb::engine_wait(e);              \
        if (_rc) return _rc;                               \
    } while (0)

namespace ukfb {

inline int fail(int code, const char* msg) {
    set_error_text(msg);
    return code;
}
inline int fail(const ukfb::Verdict& v) {
    if (v.rc != UKFB_OK) set_error_text(v.msg ? v.msg : "invalid argument");
    return v.rc;
}

// UKFB_OK, or the refusal of an engine one of whose bounded waits gave up (every entry point decides where it asks)
inline int refuse_poisoned(const ukfb_engine* e) {
    if (e->poisoned) return fail(UKFB_ERR_HIP, "engine poisoned by an earlier wait that timed out (UKFB_WAIT_TIMEOUT_S)");
    return UKFB_OK;
}

// the first lines of an entry point that refuses a poisoned engine before it looks at its arguments
inline int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return refuse_poisoned(e);
}

struct DevTmp {   // device scratch that is released on every exit path
    void* p = nullptr;
    DevTmp() = default;
    DevTmp(DevTmp&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevTmp(const DevTmp&) = delete;
    DevTmp& operator=(const DevTmp&) = delete;
    ~DevTmp() { if (p) (void)hipFree(p); }
};

// The bounded polling waits (ukfb::wait_polling, ukf_host.hpp) on a stream or an event of the engine: UKFB_OK, or UKFB_ERR_HIP
// with the text written -- `what` and the HIP error, or "timed out ..." after a wait that gave up, which also poisons the engine.
int wait_stream(ukfb_engine* e, hipStream_t s, const char* what);
int wait_event(ukfb_engine* e, hipEvent_t ev, const char* what);
int engine_wait(ukfb_engine* e);   // refuses a poisoned engine, then waits for the engine's stream

bool range_ok(const ukfb_engine* e, int64_t first, int64_t count);
int check_meas_model(const ukfb_engine* e, int m);

// host doubles <-> a device array in engine precision (elem_offset scalars into it); every one of them waits for the stream
int upload(ukfb_engine* e, void* dst_dev, size_t elem_offset, const double* src, size_t n);
int download(ukfb_engine* e, const void* src_dev, size_t elem_offset, double* dst, size_t n);
int upload_on_copy_stream(ukfb_engine* e, void* dst_dev, const double* src, size_t n);
int ensure_scratch(ukfb_engine* e, size_t bytes);
int fill_scalar(ukfb_engine* e, void* dst_dev, size_t n, double value);

template <class P> int upload_raw(ukfb_engine* e, P* dst_dev, const P* src, size_t n) {
    if (n == 0) return UKFB_OK;
    HIP_TRY(hipMemcpyAsync(dst_dev, src, n * sizeof(P), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    ENGINE_SYNC(e);
    return UKFB_OK;
}

template <class P> int download_raw(ukfb_engine* e, const P* src_dev, P* dst, size_t n) {
    if (n == 0) return UKFB_OK;
    HIP_TRY(hipMemcpyAsync(dst, src_dev, n * sizeof(P), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
    ENGINE_SYNC(e);
    return UKFB_OK;
}

int launch(ukfb_engine* e, const ukfb::LaunchReq& r);
int build_model_buckets(ukfb_engine* e, const int32_t* meas_dev, int64_t* items);
int rebuild_racc(ukfb_engine* e);
int launch_assign(ukfb_engine* e, const ukfb_assign_in& in, const ukfb_assign_out& out);   // checked arguments (ukf_assign_launch.hip)
int launch_jpda(ukfb_engine* e, const ukfb_jpda_in& in, const ukfb_pda_rule& rule, const ukfb_jpda_out& out);   // checked arguments (ukf_jpda_launch.hip)

// mount and point of a sensor-frame form (ukfb_sensor_in, ukfb_associate_in): r = 0, qs the identity and b = 0, unless the
// caller says otherwise
template <class In>
inline void set_mount_point_uniform(In* in, const double* mount_uniform, const double* point_uniform) {
    in->mount_uniform[6] = 1.0;
    if (mount_uniform) std::copy_n(mount_uniform, 7, in->mount_uniform);
    if (point_uniform) std::copy_n(point_uniform, 3, in->point_uniform);
}

// The temporaries and the copies of ONE call of a host-array form.  An array is described once, host pointer and element
// count, and the method returns its device pointer: an input is allocated and uploaded there and then, an output is allocated
// and noted for finish(), which downloads the outputs in the order they were described and drains the stream.  A NULL host
// pointer gives a NULL device pointer and allocates nothing.  The first failure is latched (rc()): every later method then
// does nothing and returns NULL, so a form asks once before its device call and once through finish().  Everything is freed
// when the stage goes out of scope, on every path (hipFree waits for the device).  The scalars cross with upload / download,
// as every other host array of the engine does.
class HostStage {
public:
    explicit HostStage(ukfb_engine* e) : e_(e) {}
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;

    int rc() const { return rc_; }

    // scalars: host doubles <-> engine precision.  zeroed: the device buffer starts as zeros (rows the kernel never writes)
    void* in(const double* h, size_t n) { return scalars(h, nullptr, n, 0, false); }
    void* out(double* h, size_t n, bool zeroed = false) { return scalars(nullptr, h, n, 0, zeroed); }
    void* inout(double* h, size_t n) { return scalars(h, h, n, 0, false); }
    // covariances: [count][D][D] row-major on the host <-> the packed lower triangle [count][PK] on the device
    void* cov_in(const double* h, size_t count) { return scalars(h, nullptr, count, e_->D, false); }
    void* cov_out(double* h, size_t count, bool zeroed = false) { return scalars(nullptr, h, count, e_->D, zeroed); }
    void* cov_inout(double* h, size_t count) { return scalars(h, h, count, e_->D, false); }
    // typed arrays that cross as they are: int32_t, uint32_t, int64_t, uint8_t
    template <class T>
    T* raw_in(const T* h, size_t n) {
        void* d = h ? take(n * sizeof(T)) : nullptr;
        if (d) rc_ = copy_in(d, h, n * sizeof(T));
        return rc_ ? nullptr : static_cast<T*>(d);
    }
    template <class T>
    T* raw_out(T* h, size_t n) {
        void* d = h ? take(n * sizeof(T)) : nullptr;
        if (d) downloads_.push_back({d, h, n * sizeof(T), -1});
        return static_cast<T*>(d);
    }

    // every output to its host array, in the order of their description, then the stream drained
    int finish() {
        if (rc_) return rc_;
        for (const Download& j : downloads_) {
            if (j.D < 0) {
                HIP_TRY(hipMemcpyAsync(j.host, j.dev, j.n, hipMemcpyDeviceToHost, main_stream(e_)));
            } else if (j.D == 0) {
                if (const int rc = download(e_, j.dev, 0, static_cast<double*>(j.host), j.n)) return rc;
            } else {
                std::vector<double> packed(j.n * size_t(e_->PK));
                if (const int rc = download(e_, j.dev, 0, packed.data(), packed.size())) return rc;
                unpack_symmetric(packed.data(), j.n, j.D, static_cast<double*>(j.host));
            }
        }
        return ukfb_sync(e_);
    }

private:
    struct Download {   // D < 0: n bytes as they are; D == 0: n scalars; D > 0: n covariances of D x D
        void* dev;
        void* host;
        size_t n;
        int D;
    };

    void* take(size_t bytes) {   // (a zero-sized array still gets a buffer: the device forms refuse NULL for a required one)
        if (rc_) return nullptr;
        DevTmp buf;
        rc_ = alloc(&buf.p, bytes ? bytes : 1);
        if (rc_) return nullptr;
        bufs_.push_back(std::move(buf));
        return bufs_.back().p;
    }
    int alloc(void** p, size_t bytes) {
        HIP_TRY(hipMalloc(p, bytes));
        return UKFB_OK;
    }
    int copy_in(void* dst, const void* src, size_t bytes) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, main_stream(e_)));
        return UKFB_OK;
    }
    int zero(void* dst, size_t bytes) {
        HIP_TRY(hipMemsetAsync(dst, 0, bytes, main_stream(e_)));
        return UKFB_OK;
    }

    // src: uploaded now; dst: downloaded by finish(); D > 0: count covariances, packed on the device
    void* scalars(const double* src, double* dst, size_t count, int D, bool zeroed) {
        if (!src && !dst) return nullptr;
        const size_t n = D ? count * size_t(e_->PK) : count;
        void* d = take(n * e_->tsize);
        if (!d) return nullptr;
        if (src && D) {
            std::vector<double> packed(n);
            pack_lower(src, count, D, packed.data());
            rc_ = upload(e_, d, 0, packed.data(), n);
        } else if (src) {
            rc_ = upload(e_, d, 0, src, n);
        }
        if (zeroed && !rc_) rc_ = zero(d, n * e_->tsize);
        if (rc_) return nullptr;
        if (dst) downloads_.push_back({d, dst, count, D});
        return d;
    }

    ukfb_engine* e_;
    int rc_ = UKFB_OK;
    std::vector<DevTmp> bufs_;
    std::vector<Download> downloads_;
};

}  // namespace ukfb
