// ukf_events.hip -- the time-ordered asynchronous measurement stream (include/ukf_batch.h, ukfb_process_events,
// ukfb_process_events_dev): the device-side ordering of an event list and one indirect fused launch per round.  The only
// one of the host translation units (the Makefile's HOST_TUS) that includes <hipcub/hipcub.hpp>, for its device-wide sorts and scans.
#include <algorithm>
#include <cmath>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "ukf_api_common.hpp"

using namespace ukfb;

namespace {
// ---- device-side ordering of an event stream ------------------------------------------------------------
__global__ void events_init_kernel(const int64_t* filt, const int64_t* ts, int64_t n, int64_t cap, uint32_t* idx,
                                   int64_t* key_t, uint32_t* flags) {
    const int64_t k = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (k >= n) return;
    idx[k] = uint32_t(k);
    key_t[k] = ts[k];
    if (filt[k] < 0 || filt[k] >= cap || ts[k] < 0) atomicOr(&flags[0], 1u);
}
__global__ void events_filter_keys_kernel(const int64_t* filt, const uint32_t* idx, int64_t n, int64_t cap, uint32_t* key_f) {
    const int64_t k = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (k >= n) return;
    const int64_t f = filt[idx[k]];
    key_f[k] = uint32_t((f < 0 || f >= cap) ? 0 : f);
}
__global__ void events_heads_kernel(const uint32_t* key_f_sorted, int64_t n, uint32_t* head) {
    const int64_t k = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (k >= n) return;
    head[k] = (k == 0 || key_f_sorted[k] != key_f_sorted[k - 1]) ? uint32_t(k) : 0u;
}
// rank of a sample inside its filter's run = its round.  The sort key of the round-major order also carries the class of the
// sample's update (2 bits, most expensive first): inside a round the indirect launch then runs class-uniform wavefronts
// (all but the one or two that straddle a class boundary), as the model-class buckets of ukfb_cycle_dev do
__global__ void events_rank_kernel(const uint32_t* start, const uint32_t* idx, const int32_t* meas, int engine_model, int64_t n,
                                   uint32_t* key, uint32_t* flags) {
    const int64_t k = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (k >= n) return;
    const uint32_t r = uint32_t(k) - start[k];
    if (r >= (1u << 30)) atomicOr(&flags[0], 2u);   // a billion samples of one filter in one call: not representable in the key
    key[k] = (r << 2) | uint32_t(2 - ukfb::update_class(engine_model, meas[idx[k]]));
    atomicMax(&flags[1], r);
}
// first position of every round in the (rank, filter)-ordered event list; off[rounds] = n
__global__ void events_round_offsets_kernel(const uint32_t* key_sorted, int64_t n, uint32_t* off) {
    const int64_t p = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = key_sorted[p] >> 2;
    if (p == 0 || (key_sorted[p - 1] >> 2) != r) off[r] = uint32_t(p);
    if (p == n - 1) off[r + 1] = uint32_t(n);
}
// events in their final (round-major, filter-minor) order, compact and in the engine's precision: what the
// indirect launches of the fused kernel read directly (no per-round scatter, no capacity-sized staging)
template <class S, class T>
__global__ void events_gather_kernel(const int64_t* filt, const int64_t* ts, const int32_t* meas, const S* z, const S* Q,
                                     const uint32_t* order, int64_t n, int32_t* fidx_c, int64_t* ts_c, int32_t* meas_c, T* z_c,
                                     T* Q_c) {
    const int64_t p = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (p >= n) return;
    const int64_t i = order[p];
    fidx_c[p] = int32_t(filt[i]);
    ts_c[p] = ts[i];
    meas_c[p] = meas[i];
    for (int c = 0; c < 3; ++c) z_c[p * 3 + c] = T(z[i * 3 + c]);
    for (int c = 0; c < 9; ++c) Q_c[p * 9 + c] = T(Q[i * 9 + c]);
}

// Device pipeline shared by both entry points.  Events are in device memory (z, Q in precision S); everything
// else lives in the engine's grow-only workspace `ev_dev`.  Ordering: radix sort by timestamp, then stable radix
// sort by filter index (hipCUB) = per-filter time order with arrival order for equal stamps; the rank of a sample
// inside its filter's run is its round.
template <class S>
int process_events_device(ukfb_engine* e, int64_t n, const int64_t* d_f, const int64_t* d_t, const int32_t* d_m, const S* d_z,
                          const S* d_q, size_t ws_offset, uint32_t* status_or, int64_t* rounds) {
    if (e->cap > 0x7fffffff) return fail(UKFB_ERR_INVALID_ARG, "ukfb_process_events: capacity exceeds 32-bit filter indices");
    const int bits_f = std::max(1, int(std::ceil(std::log2(double(std::max<int64_t>(e->cap, 2))))));
    size_t tmp_sort_t = 0, tmp_sort_f = 0, tmp_scan = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort_t, static_cast<int64_t*>(nullptr), static_cast<int64_t*>(nullptr),
                                               static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), int(n), 0, 64,
                                               ukfb::main_stream(e)));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort_f, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                               static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), int(n), 0, 32,
                                               ukfb::main_stream(e)));
    HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, tmp_scan, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                              hipcub::Max(), int(n), ukfb::main_stream(e)));
    const size_t tmp_bytes = std::max(tmp_sort_t, std::max(tmp_sort_f, tmp_scan));
    ukfb::Carver c(static_cast<char*>(e->ev_dev) + ws_offset);
    const size_t ne = size_t(n);
    uint32_t* idx_a = c.take<uint32_t>(ne);
    uint32_t* idx_b = c.take<uint32_t>(ne);
    uint32_t* idx_c = c.take<uint32_t>(ne);
    uint32_t* idx_d = c.take<uint32_t>(ne);
    int64_t* key_t_a = c.take<int64_t>(ne);
    int64_t* key_t_b = c.take<int64_t>(ne);
    uint32_t* key_f_a = c.take<uint32_t>(ne);
    uint32_t* key_f_b = c.take<uint32_t>(ne);
    uint32_t* head = c.take<uint32_t>(ne);
    uint32_t* start = c.take<uint32_t>(ne);
    uint32_t* rank = c.take<uint32_t>(ne);
    uint32_t* rank_sorted = c.take<uint32_t>(ne);
    uint32_t* off = c.take<uint32_t>(ne + 1);
    int32_t* fidx_c = c.take<int32_t>(ne);
    int64_t* ts_c = c.take<int64_t>(ne);
    int32_t* meas_c = c.take<int32_t>(ne);
    char* z_c = c.take<char>(3 * ne * e->tsize);
    char* Q_c = c.take<char>(9 * ne * e->tsize);
    uint32_t* flags = c.take<uint32_t>(2);
    char* tmp = c.take<char>(tmp_bytes);
    if (ws_offset + c.used > e->ev_bytes) return fail(UKFB_ERR_INVALID_ARG, "ukfb_process_events: workspace too small (internal)");

    // ---- ordering, all on the device: by timestamp, then (stable) by filter = per-filter time order; the position of
    // a sample inside its filter's run is its round; then (stable) by round = round-major, filter-minor
    const int blocks = int((n + 255) / 256);
    HIP_TRY(hipMemsetAsync(flags, 0, 2 * sizeof(uint32_t), ukfb::main_stream(e)));
    hipLaunchKernelGGL(events_init_kernel, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), d_f, d_t, n, e->cap, idx_a, key_t_a, flags);
    size_t tb = tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tb, key_t_a, key_t_b, idx_a, idx_b, int(n), 0, 64, ukfb::main_stream(e)));
    hipLaunchKernelGGL(events_filter_keys_kernel, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), d_f, idx_b, n, e->cap, key_f_a);
    tb = tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tb, key_f_a, key_f_b, idx_b, idx_c, int(n), 0, bits_f, ukfb::main_stream(e)));
    hipLaunchKernelGGL(events_heads_kernel, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), key_f_b, n, head);
    tb = tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::InclusiveScan(tmp, tb, head, start, hipcub::Max(), int(n), ukfb::main_stream(e)));
    hipLaunchKernelGGL(events_rank_kernel, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), start, idx_c, d_m, e->model, n, rank, flags);
    tb = tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tb, rank, rank_sorted, idx_c, idx_d, int(n), 0, 32, ukfb::main_stream(e)));
    hipLaunchKernelGGL(events_round_offsets_kernel, dim3(blocks), dim3(256), 0, ukfb::main_stream(e), rank_sorted, n, off);
    if (e->prec == UKFB_F64)
        hipLaunchKernelGGL((events_gather_kernel<S, double>), dim3(blocks), dim3(256), 0, ukfb::main_stream(e), d_f, d_t, d_m, d_z, d_q, idx_d,
                           n, fidx_c, ts_c, meas_c, reinterpret_cast<double*>(z_c), reinterpret_cast<double*>(Q_c));
    else
        hipLaunchKernelGGL((events_gather_kernel<S, float>), dim3(blocks), dim3(256), 0, ukfb::main_stream(e), d_f, d_t, d_m, d_z, d_q, idx_d,
                           n, fidx_c, ts_c, meas_c, reinterpret_cast<float*>(z_c), reinterpret_cast<float*>(Q_c));
    HIP_TRY(hipGetLastError());
    // ---- the one host read of the call: input validity, number of rounds and where each round starts (launch
    // geometry has to be known on the host)
    uint32_t hflags[2] = {0, 0};
    int rc = download_raw(e, flags, hflags, 2);
    if (rc) return rc;
    if (hflags[0] & 1u) return fail(UKFB_ERR_OUT_OF_RANGE, "ukfb_process_events: filter index or timestamp out of range");
    if (hflags[0] & 2u) return fail(UKFB_ERR_OUT_OF_RANGE, "ukfb_process_events: more than 2^30 samples of one filter in one call");
    const int64_t nrounds = int64_t(hflags[1]) + 1;
    std::vector<uint32_t> hoff(size_t(nrounds) + 1);
    rc = download_raw(e, off, hoff.data(), hoff.size());
    if (rc) return rc;

    // ---- one indirect fused launch per round over exactly the filters that have a sample in it: the cost of the
    // call follows the number of events, not rounds x capacity.  Status words accumulate (OR) across rounds.
    HIP_TRY(hipMemsetAsync(e->status, 0, size_t(e->cap) * sizeof(uint32_t), ukfb::main_stream(e)));
    for (int64_t r = 0; r < nrounds; ++r) {
        const size_t o = hoff[size_t(r)], cnt = size_t(hoff[size_t(r) + 1]) - o;
        if (cnt == 0) continue;
        ukfb::LaunchReq q;
        q.do_predict = true;
        q.do_update = true;
        q.ts_dev = ts_c + o;
        q.meas_dev = meas_c + o;
        q.z_dev = z_c + 3 * o * e->tsize;
        q.Q_dev = Q_c + 9 * o * e->tsize;
        q.filter_index_dev = fidx_c + o;
        q.n_items = int64_t(cnt);
        q.status_accumulate = true;
        rc = launch(e, q);
        if (rc) return rc;
    }
    if (rounds) *rounds = nrounds;
    if (status_or) return ukfb_get_status_summary(e, status_or);
    return UKFB_OK;
}

int ensure_events_arena(ukfb_engine* e, size_t bytes) {
    if (bytes <= e->ev_bytes) return UKFB_OK;
    if (e->ev_dev) HIP_TRY(hipFree(e->ev_dev));
    e->ev_dev = nullptr;
    e->ev_bytes = 0;
    HIP_TRY(hipMalloc(&e->ev_dev, bytes));
    e->ev_bytes = bytes;
    return UKFB_OK;
}
}  // namespace

extern "C" {

int ukfb_process_events(ukfb_engine* e, int64_t n_events, const int64_t* filter, const int64_t* ts_us,
                        const int32_t* meas_model, const double* z, const double* Q, uint32_t* status_or, int64_t* rounds) {
    if (!e || n_events < 0 || n_events > 0x7fffffff || (n_events > 0 && (!filter || !ts_us || !meas_model || !z || !Q)))
        return fail(UKFB_ERR_INVALID_ARG, "ukfb_process_events: bad argument");
    ON_DEVICE(e->device);
    if (status_or) *status_or = 0;
    if (rounds) *rounds = 0;
    if (n_events == 0) return UKFB_OK;
    // raw events go to the device as they are (one copy per array); ordering, conversion to the engine's
    // precision and the per-round scatter all happen there
    const size_t ne = size_t(n_events);
    ukfb::Carver raw(nullptr);
    raw.take<int64_t>(ne); raw.take<int64_t>(ne); raw.take<int32_t>(ne); raw.take<double>(3 * ne); raw.take<double>(9 * ne);
    int rc = ensure_events_arena(e, raw.used + ukfb::events_workspace_bytes(n_events));
    if (rc) return rc;
    ukfb::Carver c(e->ev_dev);
    int64_t* d_f = c.take<int64_t>(ne);
    int64_t* d_t = c.take<int64_t>(ne);
    int32_t* d_m = c.take<int32_t>(ne);
    double* d_z = c.take<double>(3 * ne);
    double* d_q = c.take<double>(9 * ne);
    HIP_TRY(hipMemcpyAsync(d_f, filter, ne * sizeof(int64_t), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    HIP_TRY(hipMemcpyAsync(d_t, ts_us, ne * sizeof(int64_t), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    HIP_TRY(hipMemcpyAsync(d_m, meas_model, ne * sizeof(int32_t), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    HIP_TRY(hipMemcpyAsync(d_z, z, 3 * ne * sizeof(double), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    HIP_TRY(hipMemcpyAsync(d_q, Q, 9 * ne * sizeof(double), hipMemcpyHostToDevice, ukfb::main_stream(e)));
    rc = process_events_device<double>(e, n_events, d_f, d_t, d_m, d_z, d_q, c.used, status_or, rounds);
    ENGINE_SYNC(e);   // the caller's buffers are free again
    return rc;
}

int ukfb_process_events_dev(ukfb_engine* e, int64_t n_events, const int64_t* filter_dev, const int64_t* ts_us_dev,
                            const int32_t* meas_model_dev, const void* z_dev, const void* Q_dev, uint32_t* status_or,
                            int64_t* rounds) {
    if (!e || n_events < 0 || n_events > 0x7fffffff ||
        (n_events > 0 && (!filter_dev || !ts_us_dev || !meas_model_dev || !z_dev || !Q_dev)))
        return fail(UKFB_ERR_INVALID_ARG, "ukfb_process_events_dev: bad argument");
    ON_DEVICE(e->device);
    if (status_or) *status_or = 0;
    if (rounds) *rounds = 0;
    if (n_events == 0) return UKFB_OK;
    int rc = ensure_events_arena(e, ukfb::events_workspace_bytes(n_events));
    if (rc) return rc;
    if (e->prec == UKFB_F64)
        return process_events_device<double>(e, n_events, filter_dev, ts_us_dev, meas_model_dev, static_cast<const double*>(z_dev),
                                             static_cast<const double*>(Q_dev), 0, status_or, rounds);
    return process_events_device<float>(e, n_events, filter_dev, ts_us_dev, meas_model_dev, static_cast<const float*>(z_dev),
                                        static_cast<const float*>(Q_dev), 0, status_or, rounds);
}

}  // extern "C"
