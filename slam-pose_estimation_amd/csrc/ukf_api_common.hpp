// ukf_api_common.hpp -- the host plumbing the feature C-ABI files share (every ukf_*_api.hip: the Makefile's FEATURES): the
// error macro, the argument verdict, the entry check with the poisoned-engine refusal, and HostStage, the one place where the
// host-array forms allocate their temporaries and copy to and from the device.  Not for ukf_batch.hip / ukf_group.hip: their
// HIP_TRY knows the timed-out wait and their fail has another signature.
#pragma once

#include <algorithm>
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

// the first lines of an entry point that refuses a poisoned engine before it looks at its arguments
inline int entry(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    return refuse_poisoned(e);
}

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
// when the stage goes out of scope, on every path (hipFree waits for the device).  The copies go through the host in engine
// precision: the host-array forms are a convenience, not a hot path.
class HostStage {
public:
    explicit HostStage(ukfb_engine* e) : e_(e) {}
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;
    ~HostStage() {
        for (void* p : bufs_) (void)hipFree(p);
    }

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
                UKFB_HIP_TRY(hipMemcpyAsync(j.host, j.dev, j.n, hipMemcpyDeviceToHost, main_stream(e_)));
            } else if (j.D == 0) {
                if (const int rc = download_scalars(j.dev, static_cast<double*>(j.host), j.n)) return rc;
            } else {
                std::vector<double> packed(j.n * size_t(e_->PK));
                if (const int rc = download_scalars(j.dev, packed.data(), packed.size())) return rc;
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
        void* p = nullptr;
        rc_ = alloc(&p, bytes ? bytes : 1);
        if (rc_) return nullptr;
        bufs_.push_back(p);
        return p;
    }
    int alloc(void** p, size_t bytes) {
        UKFB_HIP_TRY(hipMalloc(p, bytes));
        return UKFB_OK;
    }
    int copy_in(void* dst, const void* src, size_t bytes) {
        UKFB_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, main_stream(e_)));
        return UKFB_OK;
    }
    int zero(void* dst, size_t bytes) {
        UKFB_HIP_TRY(hipMemsetAsync(dst, 0, bytes, main_stream(e_)));
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
            rc_ = upload_scalars(d, packed.data(), n);
        } else if (src) {
            rc_ = upload_scalars(d, src, n);
        }
        if (zeroed && !rc_) rc_ = zero(d, n * e_->tsize);
        if (rc_) return nullptr;
        if (dst) downloads_.push_back({d, dst, count, D});
        return d;
    }

    int upload_scalars(void* dst, const double* src, size_t n) {
        if (e_->prec == UKFB_F64) {
            UKFB_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, main_stream(e_)));
            return ukfb_sync(e_);
        }
        std::vector<float> tmp(n);
        for (size_t i = 0; i < n; ++i) tmp[i] = float(src[i]);
        UKFB_HIP_TRY(hipMemcpyAsync(dst, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, main_stream(e_)));
        return ukfb_sync(e_);
    }
    int download_scalars(const void* src, double* dst, size_t n) {
        if (e_->prec == UKFB_F64) {
            UKFB_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, main_stream(e_)));
            return ukfb_sync(e_);
        }
        std::vector<float> tmp(n);
        UKFB_HIP_TRY(hipMemcpyAsync(tmp.data(), src, n * sizeof(float), hipMemcpyDeviceToHost, main_stream(e_)));
        if (const int rc = ukfb_sync(e_)) return rc;
        for (size_t i = 0; i < n; ++i) dst[i] = double(tmp[i]);
        return UKFB_OK;
    }

    ukfb_engine* e_;
    int rc_ = UKFB_OK;
    std::vector<void*> bufs_;
    std::vector<Download> downloads_;
};

}  // namespace ukfb
