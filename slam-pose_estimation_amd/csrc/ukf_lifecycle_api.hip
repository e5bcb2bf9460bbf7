// ukf_lifecycle_api.hip -- C-ABI of the filter lifecycle (include/ukf_batch.h, "filter lifecycle"): argument checks and launch
// geometry (ukf_host.hpp), the engine's lifecycle workspace, the launches of ukf_lifecycle.hpp, and the host-array forms.
#include "ukf_api_common.hpp"
#include "ukf_lifecycle.hpp"

namespace {

ukfb::LifecycleArrays arrays_of(const ukfb_engine* e) {
    ukfb::LifecycleArrays a;
    a.mu = e->mu;
    a.cov = e->cov;
    a.status = e->status;
    a.init = e->init;
    a.last_ts = e->last_ts;
    a.in_a = e->in_a;
    a.in_b = e->in_b;
    a.in_a_read = e->in_a_bound ? e->in_a_bound : e->in_a;
    a.in_b_read = e->in_b_bound ? e->in_b_bound : e->in_b;
    a.Rn = e->Rn;
    a.Racc = e->model == UKFB_MODEL_POSE ? e->Racc : nullptr;
    a.acc_cov9 = e->acc_cov_dev;
    a.cap = e->cap;
    a.S = e->S;
    a.PK = e->PK;
    a.D = e->D;
    a.noise_per_filter = e->Rn_per_filter ? 1 : 0;
    return a;
}

// The engine's workspace: created by its first lifecycle call, one allocation, published only when it is complete (the owner
// array's fill is enqueued on the engine's stream before any kernel can read it).  No later call allocates.
int workspace(ukfb_engine* e, ukfb::LifecycleWorkspace* ws) {
    const ukfb::LifecycleGeometry geo = ukfb::lifecycle_geometry(e->cap, 1);
    if (!e->lifecycle_ws) {
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, geo.ws_words * sizeof(uint32_t)));
        const hipError_t err = hipMemsetAsync(static_cast<uint32_t*>(p) + geo.owner_off, 0xff, size_t(e->cap) * sizeof(uint32_t), ukfb::main_stream(e));
        if (err != hipSuccess) {
            (void)hipFree(p);
            ukfb::set_error("lifecycle workspace: hipMemsetAsync", err);
            return UKFB_ERR_HIP;
        }
        e->lifecycle_ws = p;
    }
    uint32_t* const w = static_cast<uint32_t*>(e->lifecycle_ws);
    ws->owner = w + geo.owner_off;
    ws->counts = w + geo.counts_off;
    ws->before = w + geo.before_off;
    ws->totals = w + geo.totals_off;
    ws->hole = reinterpret_cast<int32_t*>(w + geo.hole_off);
    ws->mover = reinterpret_cast<int32_t*>(w + geo.mover_off);
    return UKFB_OK;
}

}  // namespace

extern "C" {

int ukfb_gather_filters_dev(ukfb_engine* e, int64_t n, const int32_t* index_dev, const ukfb_filter_records* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_lifecycle_args(e->cap, n, out != nullptr, false, false, false, false, e->Rn_per_filter))) return rc;
    if (n == 0) return UKFB_OK;
    ON_DEVICE(e->device);
    ukfb::LifecycleWorkspace ws;   // (gather needs none of it; the first lifecycle call of an engine creates it whichever it is)
    if (const int rc = workspace(e, &ws)) return rc;
    const dim3 grid(unsigned(ukfb::lifecycle_record_blocks(n))), block(ukfb::LC_THREADS);
    if (e->prec == UKFB_F64)
        hipLaunchKernelGGL(ukfb::ukf_lifecycle_gather_kernel<double>, grid, block, 0, ukfb::main_stream(e), arrays_of(e), n, index_dev, *out);
    else
        hipLaunchKernelGGL(ukfb::ukf_lifecycle_gather_kernel<float>, grid, block, 0, ukfb::main_stream(e), arrays_of(e), n, index_dev, *out);
    return ukfb::launch_status("ukfb_gather_filters_dev");
}

int ukfb_scatter_filters_dev(ukfb_engine* e, int64_t n, const int32_t* index_dev, const ukfb_filter_records* in) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_lifecycle_args(e->cap, n, in != nullptr, true, in && in->mu, in && in->cov_packed, in && in->noise,
                                                             e->Rn_per_filter)))
        return rc;
    if (n == 0) return UKFB_OK;
    ON_DEVICE(e->device);
    ukfb::LifecycleWorkspace ws;
    if (const int rc = workspace(e, &ws)) return rc;
    hipStream_t s = ukfb::main_stream(e);
    hipLaunchKernelGGL(ukfb::ukf_lifecycle_claim_kernel, dim3(unsigned(ukfb::lifecycle_item_blocks(n))), dim3(ukfb::LC_THREADS), 0, s, n, e->cap, index_dev,
                       ws.owner);
    const dim3 grid(unsigned(ukfb::lifecycle_record_blocks(n))), block(ukfb::LC_THREADS);
    if (e->prec == UKFB_F64)
        hipLaunchKernelGGL(ukfb::ukf_lifecycle_scatter_kernel<double>, grid, block, 0, s, arrays_of(e), n, index_dev, *in, ws.owner);
    else
        hipLaunchKernelGGL(ukfb::ukf_lifecycle_scatter_kernel<float>, grid, block, 0, s, arrays_of(e), n, index_dev, *in, ws.owner);
    return ukfb::launch_status("ukfb_scatter_filters_dev");
}

int ukfb_retire_dev(ukfb_engine* e, const uint8_t* retire_mask_dev) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (!retire_mask_dev) return ukfb::fail({UKFB_ERR_INVALID_ARG, "retire_mask_dev must not be NULL"});
    ON_DEVICE(e->device);
    ukfb::LifecycleWorkspace ws;
    if (const int rc = workspace(e, &ws)) return rc;
    hipLaunchKernelGGL(ukfb::ukf_lifecycle_retire_kernel, dim3(unsigned(ukfb::lifecycle_item_blocks(e->cap))), dim3(ukfb::LC_THREADS), 0, ukfb::main_stream(e),
                       e->cap, retire_mask_dev, e->init, e->last_ts);
    return ukfb::launch_status("ukfb_retire_dev");
}

int ukfb_compact_dev(ukfb_engine* e, int group, int32_t* new_index_dev, int32_t* old_index_dev, int64_t* live_dev) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_compact_args(e->cap, group))) return rc;
    ON_DEVICE(e->device);
    ukfb::LifecycleWorkspace ws;
    if (const int rc = workspace(e, &ws)) return rc;
    const ukfb::LifecycleGeometry geo = ukfb::lifecycle_geometry(e->cap, group);
    hipStream_t s = ukfb::main_stream(e);
    const dim3 block(ukfb::LC_THREADS), cgrid(unsigned(geo.count_blocks));
    hipLaunchKernelGGL(ukfb::ukf_lifecycle_count_kernel, cgrid, block, 0, s, static_cast<const uint8_t*>(e->init), geo.groups, group, ws.counts);
    hipLaunchKernelGGL(ukfb::ukf_lifecycle_scan_kernel, dim3(1), block, 0, s, static_cast<const uint32_t*>(ws.counts), geo.count_blocks,
                       static_cast<const uint8_t*>(e->init), geo.groups, group, ws.before, ws.totals);
    hipLaunchKernelGGL(ukfb::ukf_lifecycle_rank_kernel, cgrid, block, 0, s, static_cast<const uint8_t*>(e->init), geo.groups, group,
                       static_cast<const uint32_t*>(ws.before), static_cast<const uint32_t*>(ws.totals), ws.hole, ws.mover, geo.pair_cap, new_index_dev,
                       old_index_dev, live_dev);
    const dim3 mgrid(unsigned(geo.move_blocks));
    if (e->prec == UKFB_F64)
        hipLaunchKernelGGL(ukfb::ukf_lifecycle_move_kernel<double>, mgrid, block, 0, s, arrays_of(e), group, static_cast<const uint32_t*>(ws.totals),
                           static_cast<const int32_t*>(ws.hole), static_cast<const int32_t*>(ws.mover), new_index_dev, old_index_dev);
    else
        hipLaunchKernelGGL(ukfb::ukf_lifecycle_move_kernel<float>, mgrid, block, 0, s, arrays_of(e), group, static_cast<const uint32_t*>(ws.totals),
                           static_cast<const int32_t*>(ws.hole), static_cast<const int32_t*>(ws.mover), new_index_dev, old_index_dev);
    return ukfb::launch_status("ukfb_compact_dev");
}

int ukfb_gather_filters(ukfb_engine* e, int64_t n, const int32_t* index, double* mu, double* cov, int64_t* last_ts_us, uint8_t* initialised) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_lifecycle_args(e->cap, n, true, false, false, false, false, e->Rn_per_filter))) return rc;
    if (n == 0) return UKFB_OK;
    ON_DEVICE(e->device);
    const size_t m = size_t(n);
    ukfb::HostStage stage(e);
    const int32_t* idx_d = stage.raw_in(index, m);
    ukfb_filter_records rec{};
    rec.mu = stage.out(mu, m * size_t(e->S));
    rec.cov_packed = stage.cov_out(cov, m);
    rec.last_ts_us = stage.raw_out(last_ts_us, m);
    rec.initialised = stage.raw_out(initialised, m);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_gather_filters_dev(e, n, idx_d, &rec)) return rc;
    return stage.finish();
}

int ukfb_scatter_filters(ukfb_engine* e, int64_t n, const int32_t* index, const double* mu, const double* cov, const int64_t* last_ts_us,
                         const uint8_t* initialised, uint32_t* status) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_lifecycle_args(e->cap, n, true, true, mu != nullptr, cov != nullptr, false, e->Rn_per_filter))) return rc;
    if (n == 0) return UKFB_OK;
    ON_DEVICE(e->device);
    const size_t m = size_t(n);
    ukfb::HostStage stage(e);
    const int32_t* idx_d = stage.raw_in(index, m);
    ukfb_filter_records rec{};
    rec.mu = stage.in(mu, m * size_t(e->S));
    rec.cov_packed = stage.cov_in(cov, m);
    rec.last_ts_us = stage.raw_in(last_ts_us, m);
    rec.initialised = stage.raw_in(initialised, m);
    rec.status = stage.raw_out(status, m);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_scatter_filters_dev(e, n, idx_d, &rec)) return rc;
    return stage.finish();
}

int ukfb_compact(ukfb_engine* e, int group, int32_t* new_index, int32_t* old_index, int64_t* live) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_compact_args(e->cap, group))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap);
    ukfb::HostStage stage(e);
    int32_t* new_d = stage.raw_out(new_index, n);
    int32_t* old_d = stage.raw_out(old_index, n);
    int64_t* live_d = stage.raw_out(live, 1);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = ukfb_compact_dev(e, group, new_d, old_d, live_d)) return rc;
    return stage.finish();
}

}  // extern "C"
