// ukf_batch.hip -- the engine itself behind the C-ABI declared in include/ukf_batch.h: create / destroy / configuration,
// initialize / get_state / status, process noise, latched inputs, the body-state adapters, launch info and the timer.
//
// Host-side plumbing only: device allocation, AoS(double, full covariance) <-> device (engine
// precision, packed lower triangle) conversion, latched inputs.  The hot path's entry points are in ukf_cycle_api.hip, the
// event stream in ukf_events.hip, the model-class buckets in ukf_buckets.hip; the error channel, the waits and the transfers
// in ukf_runtime.hip (ukf_api_common.hpp).  All arithmetic
// of the hot path is in ukf_kernel.hpp.  There is deliberately NO CPU fallback: without a HIP
// device ukfb_create fails with UKFB_ERR_NO_DEVICE.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>

#include "ukf_api_common.hpp"

using namespace ukfb;

namespace {
// The covariance tiles of the OrientationState kernels are 3 x 3 on a 13 x 13 matrix: a lane whose tile hangs over the edge (rows 13,
// 14) loads its noise entries with immediate offsets from the tile origin like every other lane and drops them -- up to 2 * 13 + 2
// scalars past the last table.  Every noise allocation carries that many spare scalars (never written, never used).
constexpr size_t NOISE_TABLE_PAD = 32;

// full D x D host covariances (double, row-major) <-> the engine's packed lower triangle (precision T), on the device:
// one thread per scalar.  Replaces single-threaded host loops over count * D * D values in initialize / get_state.
template <class T> __global__ void pack_cov_kernel(const double* full, T* packed, int64_t count, int D, int PK) {
    const int64_t gid = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (gid >= count * PK) return;
    const int64_t i = gid / PK;
    const int e = int(gid % PK);
    int r = int((sqrtf(8.0f * float(e) + 1.0f) - 1.0f) * 0.5f);
    if (r * (r + 1) / 2 > e) --r;
    if ((r + 1) * (r + 2) / 2 <= e) ++r;
    const int c = e - r * (r + 1) / 2;
    packed[gid] = T(full[i * D * D + r * D + c]);          // the lower triangle is what Eigen's LLT reads
}
template <class T> __global__ void unpack_cov_kernel(const T* packed, double* full, int64_t count, int D, int PK) {
    const int64_t gid = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (gid >= count * D * D) return;
    const int64_t i = gid / (int64_t(D) * D);
    const int rc = int(gid % (int64_t(D) * D)), r = rc / D, c = rc % D;
    const int hi = r > c ? r : c, lo = r > c ? c : r;
    full[gid] = double(packed[i * PK + hi * (hi + 1) / 2 + lo]);
}
constexpr int64_t COV_CHUNK = 65536;   // filters per pack / unpack pass (75 MB of scratch for D = 12)

// Racc = Rn with block(6,6,3,3) = 2 acc.cov for every stored noise matrix (PoseUKF.cpp:190-191)
template <class T> __global__ void build_racc_kernel(const T* Rn, T* Racc, int64_t nmat, int D, const T* acc_cov9) {
    const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i >= nmat * D * D) return;
    const int rc = int(i % (int64_t(D) * D)), r = rc / D, c = rc % D;
    const bool vel = r >= 6 && r < 9 && c >= 6 && c < 9;
    Racc[i] = vel ? T(2) * acc_cov9[(r - 6) * 3 + (c - 6)] : Rn[i];
}
}  // namespace

int ukfb::rebuild_racc(ukfb_engine* e) {
    // the short update factorisation's host-side condition (ukfb::short_update_ok) for the batch-uniform noise
    e->noise_psd = !e->Rn_per_filter && e->Rn_host.size() == size_t(e->D) * e->D &&
                   ukfb::short_update_ok(e->model, e->D, e->Rn_host.data(), e->acc_cov);
    if (e->model != UKFB_MODEL_POSE) return UKFB_OK;
    const int64_t nmat = e->Rn_per_filter ? e->cap : 1;
    const size_t dd = size_t(e->D) * e->D;
    // both buffers persist for the life of the engine (Racc grows once, when the noise becomes per-filter)
    if (!e->Racc || e->Racc_mats < nmat) {
        if (e->Racc) {
            ENGINE_SYNC(e);
            HIP_TRY(hipFree(e->Racc));
        }
        e->Racc = nullptr;
        e->Racc_mats = 0;
        HIP_TRY(hipMalloc(&e->Racc, (size_t(nmat) * dd + NOISE_TABLE_PAD) * e->tsize));
        e->Racc_mats = nmat;
    }
    if (!e->acc_cov_dev) HIP_TRY(hipMalloc(&e->acc_cov_dev, 9 * sizeof(double)));
    int rc = upload(e, e->acc_cov_dev, 0, e->acc_cov, 9);
    if (rc) return rc;
    const int64_t total = nmat * int64_t(dd);
    const int blocks = int((total + 255) / 256);
    if (e->prec == UKFB_F64)
        hipLaunchKernelGGL(build_racc_kernel<double>, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), static_cast<const double*>(e->Rn),
                           static_cast<double*>(e->Racc), nmat, e->D, static_cast<const double*>(e->acc_cov_dev));
    else
        hipLaunchKernelGGL(build_racc_kernel<float>, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), static_cast<const float*>(e->Rn),
                           static_cast<float*>(e->Racc), nmat, e->D, static_cast<const float*>(e->acc_cov_dev));
    HIP_TRY(hipGetLastError());
    return UKFB_OK;   // stream-ordered: the next launch on the engine's stream sees the new table
}

namespace {
// BodyStateMeasurement::toRigidBodyState for a batch: one thread per output scalar (coalesced stores).
template <class T> __global__ void export_body_states_kernel(const T* mu, const T* cov, int64_t first, int64_t count, T* out) {
    const int64_t gid = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (gid >= count * 49) return;
    const int64_t i = gid / 49, f = first + i;
    const int j = int(gid % 49);
    const T* m = mu + f * 13;
    T v;
    if (j < 7) {
        v = m[j];                                   // position, orientation
    } else if (j < 10) {                            // velocity rotated into the navigation frame (:32)
        const T qx = m[3], qy = m[4], qz = m[5], qw = m[6];
        const T vx = m[7], vy = m[8], vz = m[9];
        T ux = qy * vz - qz * vy, uy = qz * vx - qx * vz, uz = qx * vy - qy * vx;
        ux += ux; uy += uy; uz += uz;
        const T r0 = vx + qw * ux + (qy * uz - qz * uy);
        const T r1 = vy + qw * uy + (qz * ux - qx * uz);
        const T r2 = vz + qw * uz + (qx * uy - qy * ux);
        v = (j == 7) ? r0 : ((j == 8) ? r1 : r2);
    } else if (j < 13) {
        v = m[j];                                   // angular velocity
    } else {
        const int b = (j - 13) / 9, rc = (j - 13) % 9, r = 3 * b + rc / 3, c = 3 * b + rc % 3;
        const int hi = r > c ? r : c, lo = r > c ? c : r;
        v = cov[f * 78 + hi * (hi + 1) / 2 + lo];
    }
    out[gid] = v;
}
// fromRigidBodyState + initializeFilter: one thread per stored scalar (13 mean + 78 packed covariance)
template <class T> __global__ void import_body_states_kernel(const T* in, int64_t first, int64_t count, T* mu, T* cov) {
    const int64_t gid = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (gid >= count * 91) return;
    const int64_t i = gid / 91, f = first + i;
    const int j = int(gid % 91);
    const T* rec = in + i * 49;
    if (j < 13) {
        mu[f * 13 + j] = rec[j];
    } else {
        const int e = j - 13;
        int r = int((sqrtf(8.0f * float(e) + 1.0f) - 1.0f) * 0.5f);
        if (r * (r + 1) / 2 > e) --r;
        if ((r + 1) * (r + 2) / 2 <= e) ++r;
        const int c = e - r * (r + 1) / 2;
        const bool same = (r / 3) == (c / 3);
        const T v = same ? rec[13 + (r / 3) * 9 + (r % 3) * 3 + (c % 3)] : T(0);
        cov[f * 78 + e] = v;
    }
}

template <class T> int export_body_states(ukfb_engine* e, int64_t first, int64_t count, double* out) {
    DevTmp dev;
    HIP_TRY(hipMalloc(&dev.p, size_t(count) * 49 * sizeof(T)));
    const int blocks = int((count * 49 + 255) / 256);
    hipLaunchKernelGGL(export_body_states_kernel<T>, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), static_cast<const T*>(e->mu),
                       static_cast<const T*>(e->cov), first, count, static_cast<T*>(dev.p));
    HIP_TRY(hipGetLastError());
    return download(e, dev.p, 0, out, size_t(count) * 49);
}
template <class T> int import_body_states(ukfb_engine* e, int64_t first, int64_t count, const double* in) {
    DevTmp dev;
    HIP_TRY(hipMalloc(&dev.p, size_t(count) * 49 * sizeof(T)));
    int rc = upload(e, dev.p, 0, in, size_t(count) * 49);
    if (rc) return rc;
    const int blocks = int((count * 91 + 255) / 256);
    hipLaunchKernelGGL(import_body_states_kernel<T>, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), static_cast<const T*>(dev.p), first,
                       count, static_cast<T*>(e->mu), static_cast<T*>(e->cov));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(e->init + first, 1, size_t(count), ukfb::main_stream(e)));
    HIP_TRY(hipMemsetAsync(e->last_ts + first, 0, size_t(count) * sizeof(int64_t), ukfb::main_stream(e)));
    ENGINE_SYNC(e);
    return UKFB_OK;
}

__global__ void or_reduce_kernel(const uint32_t* st, int64_t n, uint32_t* out) {
    uint32_t v = 0;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
        v |= st[i];
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicOr(out, v);
}

}  // namespace

extern "C" {

int ukfb_default_config(ukfb_config* cfg) {
    if (!cfg) return UKFB_ERR_INVALID_ARG;
    cfg->mean_tol = 1e-6;
    cfg->mean_max_iter = 10000;   // ukfom's cap; the loop is wave-uniform and leaves on convergence, the cap costs nothing
    cfg->gate_chi2 = -1.0;
    cfg->min_time_delta = 1.0e-9;
    cfg->max_time_delta = std::numeric_limits<double>::max();
    cfg->lanes_per_filter = 16;
    cfg->bucket_models = 1;
    cfg->split_streams = 1;
    cfg->wide_arithmetic = 0;
    cfg->full_update_check = 0;
    return UKFB_OK;
}

static int create_engine(ukfb_engine* e, int64_t capacity, void* stream, bool use_given_stream) {
    if (stream || use_given_stream) {
        e->stream = static_cast<hipStream_t>(stream);   // (NULL with use_given_stream: the device's default stream)
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        e->own_stream = true;
        // the second stream of split launches (see ukf_launch.inc.hpp); a caller's stream keeps plain stream order
        HIP_TRY(hipStreamCreateWithFlags(&e->stream_b, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_a, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_b, hipEventDisableTiming));
    }
    const size_t n = size_t(capacity), ts = e->tsize;
    HIP_TRY(hipMalloc(&e->mu, n * e->S * ts));
    HIP_TRY(hipMalloc(&e->cov, n * e->PK * ts));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->status), n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->init), n));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->last_ts), n * sizeof(int64_t)));
    HIP_TRY(hipMalloc(&e->Rn, (size_t(e->D) * e->D + NOISE_TABLE_PAD) * ts));
    HIP_TRY(hipMalloc(&e->in_a, n * 3 * ts));
    HIP_TRY(hipMalloc(&e->in_b, n * 3 * ts));
    HIP_TRY(hipMalloc(&e->z_stage, n * 3 * ts));
    HIP_TRY(hipMalloc(&e->Q_stage, n * 9 * ts));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->meas_stage), n * sizeof(int32_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->active_stage), n));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->dt_stage), n * sizeof(double)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->ts_stage), n * sizeof(int64_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->reduce_word), sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(e->mu, 0, n * e->S * ts, ukfb::main_stream(e)));
    HIP_TRY(hipMemsetAsync(e->cov, 0, n * e->PK * ts, ukfb::main_stream(e)));
    HIP_TRY(hipMemsetAsync(e->status, 0, n * sizeof(uint32_t), ukfb::main_stream(e)));
    HIP_TRY(hipMemsetAsync(e->init, 0, n, ukfb::main_stream(e)));
    HIP_TRY(hipMemsetAsync(e->last_ts, 0, n * sizeof(int64_t), ukfb::main_stream(e)));
    HIP_TRY(hipMemsetAsync(e->Rn, 0, size_t(e->D) * e->D * ts, ukfb::main_stream(e)));  // UnscentedKalmanFilter.hpp:29
    HIP_TRY(hipMemsetAsync(e->in_b, 0, n * 3 * ts, ukfb::main_stream(e)));
    HIP_TRY(hipMemsetAsync(e->z_stage, 0, n * 3 * ts, ukfb::main_stream(e)));
    HIP_TRY(hipMemsetAsync(e->Q_stage, 0, n * 9 * ts, ukfb::main_stream(e)));
    e->Rn_host.assign(size_t(e->D) * e->D, 0.0);
    int rc;
    if (e->model == UKFB_MODEL_POSE)  // acceleration.mu = NaN until set (PoseUKF.cpp:109)
        rc = fill_scalar(e, e->in_a, n * 3, std::numeric_limits<double>::quiet_NaN());
    else
        rc = fill_scalar(e, e->in_a, n * 3, 0.0);
    if (rc) return rc;
    HIP_TRY(hipEventCreate(&e->ev0));
    HIP_TRY(hipEventCreate(&e->ev1));
    ENGINE_SYNC(e);
    return rebuild_racc(e);
}

static int create_impl(ukfb_engine** out, int model, int precision, int64_t capacity, int device, void* stream,
                       bool use_given_stream) {
    if (!out || capacity <= 0 || (model != UKFB_MODEL_POSE && model != UKFB_MODEL_ORIENT) ||
        (precision != UKFB_F64 && precision != UKFB_F32))
        return fail(UKFB_ERR_INVALID_ARG, "ukfb_create: bad argument");
    *out = nullptr;
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        return fail(UKFB_ERR_NO_DEVICE, "ukfb_create: no usable HIP device (the engine has no CPU fallback)");
    }
    ON_DEVICE(device);
    ukfb_engine* e = new (std::nothrow) ukfb_engine();
    if (!e) return fail(UKFB_ERR_INVALID_ARG, "out of host memory");
    e->model = model;
    e->prec = precision;
    e->cap = capacity;
    e->device = device;
    e->S = model == UKFB_MODEL_POSE ? 13 : 14;
    e->D = model == UKFB_MODEL_POSE ? 12 : 13;
    e->PK = e->D * (e->D + 1) / 2;
    e->tsize = precision == UKFB_F64 ? 8 : 4;
    ukfb_default_config(&e->cfg);
    const int rc = create_engine(e, capacity, stream, use_given_stream);
    if (rc) {   // release the stream, the events and every buffer allocated so far; keep the error text
        const std::string msg = ukfb_last_error();
        ukfb_destroy(e);
        set_error_text(msg);
        return rc;
    }
    *out = e;
    return UKFB_OK;
}

int ukfb_create(ukfb_engine** out, int model, int precision, int64_t capacity, int device, void* stream) {
    return create_impl(out, model, precision, capacity, device, stream, false);
}

int ukfb_create_on_stream(ukfb_engine** out, int model, int precision, int64_t capacity, int device, void* stream) {
    return create_impl(out, model, precision, capacity, device, stream, true);
}

int ukfb_layout_supported(int precision, int lanes_per_filter) {
    return ukfb::layout_supported(precision, lanes_per_filter, UKFB_GENERIC_F64 != 0) ? 1 : 0;
}

int ukfb_destroy(ukfb_engine* e) {
    if (!e) return UKFB_OK;
    ukfb::DeviceScope device_scope(e->device);
    // bounded: a kernel that never finishes must not pin the host in the teardown either.  A poisoned engine (this wait or
    // an earlier one timed out) is abandoned as it is -- freeing memory under a kernel in flight would be worse than the leak
    (void)engine_wait(e);
    if (e->poisoned) {
        delete e;
        return fail(UKFB_ERR_HIP, "ukfb_destroy: the engine's stream never drained; device memory left allocated, exit the process");
    }
    void* bufs[] = {e->mu, e->cov, e->status, e->init, e->last_ts, e->Rn, e->Racc, e->acc_cov_dev, e->in_a, e->in_b, e->z_stage,
                    e->Q_stage, e->meas_stage, e->active_stage, e->dt_stage, e->ts_stage, e->reduce_word, e->ev_dev, e->cvt_dev,
                    e->multi_dev, e->bucket_idx, e->bucket_counts, e->smooth_chain, e->lifecycle_ws};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    for (int s2 = 0; s2 < 2; ++s2) {
        if (e->zc_stage[s2]) (void)hipFree(e->zc_stage[s2]);
        if (e->Qc_stage[s2]) (void)hipFree(e->Qc_stage[s2]);
        if (e->ev_copy[s2]) (void)hipEventDestroy(e->ev_copy[s2]);
        if (e->ev_used[s2]) (void)hipEventDestroy(e->ev_used[s2]);
    }
    if (e->cvt_copy) (void)hipFree(e->cvt_copy);
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    if (e->ev_a) (void)hipEventDestroy(e->ev_a);
    if (e->ev_b) (void)hipEventDestroy(e->ev_b);
    if (e->stream_b) (void)hipStreamDestroy(e->stream_b);
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return UKFB_OK;
}

int ukfb_set_config(ukfb_engine* e, const ukfb_config* cfg) {
    if (!e || !cfg) return UKFB_ERR_INVALID_ARG;
    ukfb_config c = *cfg;
    const ukfb::Verdict v = ukfb::check_config(e->prec, UKFB_GENERIC_F64 != 0, c);
    if (v.rc) return fail(v.rc, v.msg);
    e->cfg = c;
    return UKFB_OK;
}

int ukfb_get_config(const ukfb_engine* e, ukfb_config* cfg) {
    if (!e || !cfg) return UKFB_ERR_INVALID_ARG;
    *cfg = e->cfg;
    return UKFB_OK;
}

int ukfb_describe(const ukfb_engine* e, int* model, int* precision, int64_t* capacity, int* S, int* D, int* PK) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (model) *model = e->model;
    if (precision) *precision = e->prec;
    if (capacity) *capacity = e->cap;
    if (S) *S = e->S;
    if (D) *D = e->D;
    if (PK) *PK = e->PK;
    return UKFB_OK;
}

int ukfb_initialize(ukfb_engine* e, int64_t first, int64_t count, const double* mu, const double* cov) {
    if (!range_ok(e, first, count) || !mu || !cov) return fail(UKFB_ERR_OUT_OF_RANGE, "ukfb_initialize: bad range");
    ON_DEVICE(e->device);
    const int D = e->D, PK = e->PK;
    int rc = upload(e, e->mu, size_t(first) * e->S, mu, size_t(count) * e->S);
    if (rc) return rc;
    // covariances: the full matrices cross PCIe as they are, the packing (and narrowing) runs on the device
    for (int64_t lo = 0; lo < count; lo += COV_CHUNK) {
        const int64_t m = std::min(COV_CHUNK, count - lo);
        const size_t nfull = size_t(m) * D * D;
        rc = ensure_scratch(e, nfull * sizeof(double));
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(e->cvt_dev, cov + size_t(lo) * D * D, nfull * sizeof(double), hipMemcpyHostToDevice, ukfb::main_stream(e)));
        const unsigned blocks = unsigned((size_t(m) * PK + 255) / 256);
        if (e->prec == UKFB_F64)
            hipLaunchKernelGGL(pack_cov_kernel<double>, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), static_cast<const double*>(e->cvt_dev),
                               static_cast<double*>(e->cov) + size_t(first + lo) * PK, m, D, PK);
        else
            hipLaunchKernelGGL(pack_cov_kernel<float>, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), static_cast<const double*>(e->cvt_dev),
                               static_cast<float*>(e->cov) + size_t(first + lo) * PK, m, D, PK);
        HIP_TRY(hipGetLastError());
        ENGINE_SYNC(e);   // the scratch is reused by the next chunk
    }
    HIP_TRY(hipMemsetAsync(e->init + first, 1, size_t(count), ukfb::main_stream(e)));
    HIP_TRY(hipMemsetAsync(e->last_ts + first, 0, size_t(count) * sizeof(int64_t), ukfb::main_stream(e)));
    ENGINE_SYNC(e);
    return UKFB_OK;
}

int ukfb_get_state(ukfb_engine* e, int64_t first, int64_t count, double* mu, double* cov, uint8_t* initialised) {
    if (!range_ok(e, first, count)) return fail(UKFB_ERR_OUT_OF_RANGE, "ukfb_get_state: bad range");
    ON_DEVICE(e->device);
    const int D = e->D, PK = e->PK;
    int rc;
    if (mu) {
        rc = download(e, e->mu, size_t(first) * e->S, mu, size_t(count) * e->S);
        if (rc) return rc;
    }
    if (cov) {   // mirrored to full matrices (and widened) on the device, chunk by chunk
        for (int64_t lo = 0; lo < count; lo += COV_CHUNK) {
            const int64_t m = std::min(COV_CHUNK, count - lo);
            const size_t nfull = size_t(m) * D * D;
            rc = ensure_scratch(e, nfull * sizeof(double));
            if (rc) return rc;
            const unsigned blocks = unsigned((nfull + 255) / 256);
            if (e->prec == UKFB_F64)
                hipLaunchKernelGGL(unpack_cov_kernel<double>, dim3(blocks), dim3(256), 0, ukfb::main_stream(e),
                                   static_cast<const double*>(e->cov) + size_t(first + lo) * PK, static_cast<double*>(e->cvt_dev), m, D, PK);
            else
                hipLaunchKernelGGL(unpack_cov_kernel<float>, dim3(blocks), dim3(256), 0, ukfb::main_stream(e),
                                   static_cast<const float*>(e->cov) + size_t(first + lo) * PK, static_cast<double*>(e->cvt_dev), m, D, PK);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(cov + size_t(lo) * D * D, e->cvt_dev, nfull * sizeof(double), hipMemcpyDeviceToHost, ukfb::main_stream(e)));
            ENGINE_SYNC(e);
        }
    }
    if (initialised) {
        rc = download_raw(e, e->init + first, initialised, size_t(count));
        if (rc) return rc;
    }
    return UKFB_OK;
}

int ukfb_get_status(ukfb_engine* e, int64_t first, int64_t count, uint32_t* status) {
    if (!range_ok(e, first, count) || !status) return fail(UKFB_ERR_OUT_OF_RANGE, "ukfb_get_status: bad range");
    ON_DEVICE(e->device);
    return download_raw(e, e->status + first, status, size_t(count));
}

int ukfb_get_status_summary(ukfb_engine* e, uint32_t* or_of_all) {
    if (!e || !or_of_all) return UKFB_ERR_INVALID_ARG;
    ON_DEVICE(e->device);
    HIP_TRY(hipMemsetAsync(e->reduce_word, 0, sizeof(uint32_t), ukfb::main_stream(e)));
    const int blocks = int(std::min<int64_t>((e->cap + 255) / 256, 1024));
    hipLaunchKernelGGL(or_reduce_kernel, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), e->status, e->cap, e->reduce_word);
    HIP_TRY(hipGetLastError());
    return download_raw(e, e->reduce_word, or_of_all, 1);
}

int ukfb_set_last_measurement_time(ukfb_engine* e, int64_t first, int64_t count, const int64_t* t_us) {
    if (!range_ok(e, first, count) || !t_us) return fail(UKFB_ERR_OUT_OF_RANGE, "bad range");
    ON_DEVICE(e->device);
    return upload_raw(e, e->last_ts + first, t_us, size_t(count));
}

int ukfb_get_last_measurement_time(ukfb_engine* e, int64_t first, int64_t count, int64_t* t_us) {
    if (!range_ok(e, first, count) || !t_us) return fail(UKFB_ERR_OUT_OF_RANGE, "bad range");
    ON_DEVICE(e->device);
    return download_raw(e, e->last_ts + first, t_us, size_t(count));
}

int ukfb_device_views(ukfb_engine* e, void** mu_dev, void** cov_packed_dev, uint32_t** status_dev) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (mu_dev) *mu_dev = e->mu;
    if (cov_packed_dev) *cov_packed_dev = e->cov;
    if (status_dev) *status_dev = e->status;
    return UKFB_OK;
}

int ukfb_set_process_noise(ukfb_engine* e, const double* R) {
    if (!e || !R) return UKFB_ERR_INVALID_ARG;
    ON_DEVICE(e->device);
    const size_t dd = size_t(e->D) * e->D;
    e->Rn_host.assign(R, R + dd);
    e->noise_iso = ukfb::rotated_blocks_isotropic(R, e->D);
    if (e->Rn_per_filter) {
        std::vector<double> all(size_t(e->cap) * dd);
        for (int64_t i = 0; i < e->cap; ++i) std::memcpy(all.data() + size_t(i) * dd, R, dd * sizeof(double));
        int rc = upload(e, e->Rn, 0, all.data(), all.size());
        return rc ? rc : rebuild_racc(e);
    }
    int rc = upload(e, e->Rn, 0, R, dd);
    return rc ? rc : rebuild_racc(e);
}

int ukfb_set_process_noise_per_filter(ukfb_engine* e, int64_t first, int64_t count, const double* R) {
    if (!range_ok(e, first, count) || !R) return fail(UKFB_ERR_OUT_OF_RANGE, "bad range");
    ON_DEVICE(e->device);
    const size_t dd = size_t(e->D) * e->D;
    if (!e->Rn_per_filter) {
        void* big = nullptr;
        HIP_TRY(hipMalloc(&big, (size_t(e->cap) * dd + NOISE_TABLE_PAD) * e->tsize));
        ENGINE_SYNC(e);
        HIP_TRY(hipFree(e->Rn));
        e->Rn = big;
        e->Rn_per_filter = true;
        std::vector<double> all(size_t(e->cap) * dd);
        for (int64_t i = 0; i < e->cap; ++i)
            std::memcpy(all.data() + size_t(i) * dd, e->Rn_host.data(), dd * sizeof(double));
        int rc = upload(e, e->Rn, 0, all.data(), all.size());
        if (rc) return rc;
    }
    int rc = upload(e, e->Rn, size_t(first) * dd, R, size_t(count) * dd);
    return rc ? rc : rebuild_racc(e);
}

int ukfb_get_process_noise(ukfb_engine* e, int64_t filter, double* R) {
    if (!range_ok(e, filter, 1) || !R) return fail(UKFB_ERR_OUT_OF_RANGE, "bad range");
    ON_DEVICE(e->device);
    const size_t dd = size_t(e->D) * e->D;
    return download(e, e->Rn, e->Rn_per_filter ? size_t(filter) * dd : 0, R, dd);
}

int ukfb_pose_set_acceleration(ukfb_engine* e, int64_t first, int64_t count, const double* acc_mu,
                               const double* acc_cov) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (e->model != UKFB_MODEL_POSE) return fail(UKFB_ERR_WRONG_MODEL, "Pose engines only");
    if (!range_ok(e, first, count)) return fail(UKFB_ERR_OUT_OF_RANGE, "bad range");
    ON_DEVICE(e->device);
    if (acc_cov) {
        std::memcpy(e->acc_cov, acc_cov, 9 * sizeof(double));
        int rc = rebuild_racc(e);
        if (rc) return rc;
    }
    if (acc_mu) return upload(e, e->in_a, size_t(first) * 3, acc_mu, size_t(count) * 3);
    return UKFB_OK;
}

int ukfb_pose_bind_acceleration_dev(ukfb_engine* e, const void* acc_mu_dev) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (e->model != UKFB_MODEL_POSE) return fail(UKFB_ERR_WRONG_MODEL, "Pose engines only");
    e->in_a_bound = acc_mu_dev;
    return UKFB_OK;
}

int ukfb_orient_set_params(ukfb_engine* e, double gyro_bias_tau, double acc_bias_tau, const double earth_rotation[3]) {
    if (!e || !earth_rotation) return UKFB_ERR_INVALID_ARG;
    if (e->model != UKFB_MODEL_ORIENT) return fail(UKFB_ERR_WRONG_MODEL, "Orient engines only");
    e->tau_g = gyro_bias_tau;
    e->tau_a = acc_bias_tau;
    for (int k = 0; k < 3; ++k) e->earth[k] = earth_rotation[k];
    return UKFB_OK;
}

int ukfb_orient_set_inputs(ukfb_engine* e, int64_t first, int64_t count, const double* gyro, const double* acc) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (e->model != UKFB_MODEL_ORIENT) return fail(UKFB_ERR_WRONG_MODEL, "Orient engines only");
    if (!range_ok(e, first, count)) return fail(UKFB_ERR_OUT_OF_RANGE, "bad range");
    ON_DEVICE(e->device);
    // checkMeasurment (OrientationUKF.cpp:55,61): a non-finite row keeps the previously latched value
    auto latch = [&](void* dev, const double* src) -> int {
        bool all_finite = true;
        for (int64_t i = 0; i < count * 3 && all_finite; ++i) all_finite = std::isfinite(src[i]);
        if (all_finite) return upload(e, dev, size_t(first) * 3, src, size_t(count) * 3);
        std::vector<double> cur(static_cast<size_t>(count) * 3, 0.0);
        int rc = download(e, dev, size_t(first) * 3, cur.data(), cur.size());
        if (rc) return rc;
        std::vector<uint32_t> st(static_cast<size_t>(count), 0u);
        rc = download_raw(e, e->status + first, st.data(), st.size());
        if (rc) return rc;
        for (int64_t i = 0; i < count; ++i) {
            const double* r = src + i * 3;
            if (std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]))
                std::memcpy(cur.data() + i * 3, r, 3 * sizeof(double));
            else
                st[size_t(i)] |= UKFB_ST_ERR_NONFINITE_MEAS;
        }
        rc = upload(e, dev, size_t(first) * 3, cur.data(), cur.size());
        if (rc) return rc;
        return upload_raw(e, e->status + first, st.data(), st.size());
    };
    int rc = UKFB_OK;
    if (gyro) rc = latch(e->in_b, gyro);
    if (rc) return rc;
    if (acc) rc = latch(e->in_a, acc);
    return rc;
}

int ukfb_orient_bind_inputs_dev(ukfb_engine* e, const void* gyro_dev, const void* acc_dev) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (e->model != UKFB_MODEL_ORIENT) return fail(UKFB_ERR_WRONG_MODEL, "Orient engines only");
    e->in_b_bound = gyro_dev;
    e->in_a_bound = acc_dev;
    return UKFB_OK;
}

int ukfb_orient_get_rotation_rate(ukfb_engine* e, int64_t first, int64_t count, double* out) {
    if (!e || !out) return UKFB_ERR_INVALID_ARG;
    if (e->model != UKFB_MODEL_ORIENT) return fail(UKFB_ERR_WRONG_MODEL, "Orient engines only");
    if (!range_ok(e, first, count)) return fail(UKFB_ERR_OUT_OF_RANGE, "bad range");
    ON_DEVICE(e->device);
    // rotation_rate.mu - bias_gyro - q^-1 * earth_rotation (OrientationUKF.cpp:74-77): a read-out of
    // latched input and mean, not part of the predict/update arithmetic, evaluated host-side.
    std::vector<double> mu(size_t(count) * 14), w(size_t(count) * 3);
    int rc = download(e, e->mu, size_t(first) * 14, mu.data(), mu.size());
    if (rc) return rc;
    const void* gy = e->in_b_bound ? e->in_b_bound : e->in_b;
    rc = download(e, gy, size_t(first) * 3, w.data(), w.size());
    if (rc) return rc;
    for (int64_t i = 0; i < count; ++i) {
        const double* m = mu.data() + i * 14;
        const double n2 = m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + m[3] * m[3];
        const double q[4] = {-m[0] / n2, -m[1] / n2, -m[2] / n2, m[3] / n2};
        const double* v = e->earth;
        double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
        ux += ux; uy += uy; uz += uz;
        const double r0 = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
        const double r1 = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
        const double r2 = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
        out[i * 3 + 0] = w[size_t(i) * 3 + 0] - m[7] - r0;
        out[i * 3 + 1] = w[size_t(i) * 3 + 1] - m[8] - r1;
        out[i * 3 + 2] = w[size_t(i) * 3 + 2] - m[9] - r2;
    }
    return UKFB_OK;
}

// ---- BodyStateMeasurement adapters ----------------------------------------------------------------
int ukfb_pose_export_body_states(ukfb_engine* e, int64_t first, int64_t count, double* out) {
    if (!e || !out) return UKFB_ERR_INVALID_ARG;
    if (e->model != UKFB_MODEL_POSE) return fail(UKFB_ERR_WRONG_MODEL, "Pose engines only");
    if (!range_ok(e, first, count)) return fail(UKFB_ERR_OUT_OF_RANGE, "bad range");
    if (count == 0) return UKFB_OK;
    ON_DEVICE(e->device);
    return e->prec == UKFB_F64 ? export_body_states<double>(e, first, count, out) : export_body_states<float>(e, first, count, out);
}

int ukfb_pose_import_body_states(ukfb_engine* e, int64_t first, int64_t count, const double* in) {
    if (!e || !in) return UKFB_ERR_INVALID_ARG;
    if (e->model != UKFB_MODEL_POSE) return fail(UKFB_ERR_WRONG_MODEL, "Pose engines only");
    if (!range_ok(e, first, count)) return fail(UKFB_ERR_OUT_OF_RANGE, "bad range");
    if (count == 0) return UKFB_OK;
    ON_DEVICE(e->device);
    return e->prec == UKFB_F64 ? import_body_states<double>(e, first, count, in) : import_body_states<float>(e, first, count, in);
}

// ---- measurement of the engine ------------------------------------------------------------------
int ukfb_last_launch_info(const ukfb_engine* e, char* kernel_name, int name_capacity, int* lds_bytes,
                          int* filters_per_workgroup, int64_t* grid) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (kernel_name && name_capacity > 0) {
        std::snprintf(kernel_name, size_t(name_capacity), "%s", e->last_kernel.c_str());
    }
    if (lds_bytes) *lds_bytes = e->last_lds;
    if (filters_per_workgroup) *filters_per_workgroup = e->last_fpw;
    if (grid) *grid = e->last_grid;
    return UKFB_OK;
}

int ukfb_timer_begin(ukfb_engine* e) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    ON_DEVICE(e->device);
    HIP_TRY(hipEventRecord(e->ev0, ukfb::main_stream(e)));
    return UKFB_OK;
}

int ukfb_timer_end(ukfb_engine* e, float* elapsed_ms) {
    if (!e || !elapsed_ms) return UKFB_ERR_INVALID_ARG;
    ON_DEVICE(e->device);
    if (const int rc = refuse_poisoned(e)) return rc;
    HIP_TRY(hipEventRecord(e->ev1, ukfb::main_stream(e)));
    if (const int rc = wait_event(e, e->ev1, "waiting for the timer's event")) return rc;
    HIP_TRY(hipEventElapsedTime(elapsed_ms, e->ev0, e->ev1));
    return UKFB_OK;
}

}  // extern "C"
