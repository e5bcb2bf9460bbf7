// ukf_cycle_api.hip -- C-ABI of the hot path (include/ukf_batch.h): predict, update, the fused cycle in its uniform-Q, timestamp
// and multi-cycle forms.  Host-side plumbing only: the copy-stream path of the host-fed cycles, the staging of host
// measurement arrays, the multi-cycle plan runner, the launch requests.  All arithmetic is in ukf_kernel.hpp.
#include <algorithm>

#include "ukf_api_common.hpp"

using namespace ukfb;

namespace {
// ---- host-fed fused cycles: double-buffered staging on a copy stream ----------------------------------------------------
// ukfb_cycle / ukfb_cycle_uniform_q upload z and Q before they launch.  On the engine's own stream that upload queues
// behind the kernel of the previous call: copy and kernel alternate (1 M Pose filters fp64: 2.0 ms of PCIe + 1.1 ms of
// kernel per cycle).  Here the upload of call k + 1 runs on a separate stream into the staging set call k is not reading;
// the call returns when ITS copies have been consumed (the caller's buffers are free), not when the kernel is done.
int ensure_copy_path(ukfb_engine* e) {
    if (e->copy_stream) return UKFB_OK;
    const size_t n = size_t(e->cap), ts = e->tsize;
    // everything into locals; the engine sees the set only when all of it exists (a failure frees what was created and a
    // retry starts from nothing -- no leaked stream / events / buffers, no half-initialised handles)
    hipStream_t cs = nullptr;
    hipEvent_t evc[2] = {nullptr, nullptr}, evu[2] = {nullptr, nullptr};
    void* zs[2] = {nullptr, nullptr};
    void* qs[2] = {nullptr, nullptr};
    hipError_t err = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
    for (int s = 0; s < 2 && err == hipSuccess; ++s) {
        err = hipEventCreateWithFlags(&evc[s], hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&evu[s], hipEventDisableTiming);
        if (err == hipSuccess) err = hipMalloc(&zs[s], n * 3 * ts);
        if (err == hipSuccess) err = hipMalloc(&qs[s], n * 9 * ts);
    }
    if (err != hipSuccess) {
        for (int s = 0; s < 2; ++s) {
            if (zs[s]) (void)hipFree(zs[s]);
            if (qs[s]) (void)hipFree(qs[s]);
            if (evc[s]) (void)hipEventDestroy(evc[s]);
            if (evu[s]) (void)hipEventDestroy(evu[s]);
        }
        if (cs) (void)hipStreamDestroy(cs);
        ukfb::set_error("host-fed cycles: copy stream / staging", err);
        return UKFB_ERR_HIP;
    }
    for (int s = 0; s < 2; ++s) {
        e->ev_copy[s] = evc[s];
        e->ev_used[s] = evu[s];
        e->zc_stage[s] = zs[s];
        e->Qc_stage[s] = qs[s];
    }
    e->copy_stream = cs;
    return UKFB_OK;
}

// host-fed launch: z and Q are uploaded into a staging set on the copy stream, the kernel waits for them and frees the set behind it
int launch_staged(ukfb_engine* e, ukfb::LaunchReq r, const double* z, const double* Q, size_t nq) {
    if (!z || !Q) return fail(UKFB_ERR_INVALID_ARG, "z and Q must not be NULL");
    if (const int rc = refuse_poisoned(e)) return rc;
    int rc = ensure_copy_path(e);
    if (rc) return rc;
    const size_t nz = size_t(e->cap) * 3;
    if (e->prec == UKFB_F32) {   // scratch for the widest array of the call; z and Q pass through it one after the other
        const size_t need = std::max(nz, nq) * sizeof(double);
        if (e->cvt_copy_bytes < need) {
            HIP_TRY(hipStreamSynchronize(e->copy_stream));
            if (e->cvt_copy) HIP_TRY(hipFree(e->cvt_copy));
            e->cvt_copy = nullptr;
            e->cvt_copy_bytes = 0;
            HIP_TRY(hipMalloc(&e->cvt_copy, need));
            e->cvt_copy_bytes = need;
        }
    }
    const int s = e->stage_slot;
    e->stage_slot ^= 1;
    if (e->stage_busy[s]) HIP_TRY(hipStreamWaitEvent(e->copy_stream, e->ev_used[s], 0));   // the kernel that read this set is done
    rc = upload_on_copy_stream(e, e->zc_stage[s], z, nz);
    if (!rc) rc = upload_on_copy_stream(e, e->Qc_stage[s], Q, nq);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(e->ev_copy[s], e->copy_stream));
    // the caller's buffers are free again once the copies have been consumed: wait for the COPY stream only (bounded)
    rc = wait_stream(e, e->copy_stream, "waiting for the copy stream");
    if (rc) return rc;
    r.z_dev = e->zc_stage[s];
    r.Q_dev = e->Qc_stage[s];
    r.wait_event = e->ev_copy[s];
    r.done_event = e->ev_used[s];
    r.no_split = true;   // one kernel on the engine's stream: the done event covers all of it
    rc = launch(e, r);
    if (!rc) e->stage_busy[s] = true;
    return rc;
}

// stage host measurement arrays into the engine's device buffers
int stage_measurements(ukfb_engine* e, const double* z, const double* Q, const int32_t* meas, const uint8_t* active) {
    if (!z || !Q) return fail(UKFB_ERR_INVALID_ARG, "z and Q must not be NULL");
    int rc = upload(e, e->z_stage, 0, z, size_t(e->cap) * 3);
    if (rc) return rc;
    rc = upload(e, e->Q_stage, 0, Q, size_t(e->cap) * 9);
    if (rc) return rc;
    if (meas) {
        rc = upload_raw(e, e->meas_stage, meas, size_t(e->cap));
        if (rc) return rc;
    }
    if (active) {
        rc = upload_raw(e, e->active_stage, active, size_t(e->cap));
        if (rc) return rc;
    }
    return UKFB_OK;
}

// The launches of a multi-cycle call (ukfb::CyclePlan) over device rings [slots][capacity][...]: z, Q, the latched inputs
// (optional) and per-filter model ids (meas_dev, optional).  sched_dt / sched_model: a host schedule [cycles], or NULL and the
// uniform dt / meas_model.  A per-cycle launch reads its ring slot through the engine's bound inputs, restored afterwards.
int run_cycle_plan(ukfb_engine* e, const ukfb::CyclePlan& plan, double dt, int meas_model, const double* sched_dt,
                   const int32_t* sched_model, const int32_t* meas_dev, const void* in_a_dev, const void* in_b_dev,
                   const void* z_dev, const void* Q_dev) {
    const size_t w = e->tsize;
    const void* keep_a = e->in_a_bound;
    const void* keep_b = e->in_b_bound;
    int rc = UKFB_OK;
    for (int k = 0; k < plan.launches() && rc == UKFB_OK; ++k) {
        const ukfb::CycleLaunch c = plan[k];
        ukfb::LaunchReq r;
        r.do_predict = true;
        r.do_update = true;
        r.status_accumulate = c.status_accumulate;
        if (plan.multi) {
            r.dt_uniform = dt;
            r.meas_uniform = meas_model;
            r.meas_dev = meas_dev;
            r.z_dev = z_dev;
            r.Q_dev = Q_dev;
            r.cycles = c.cycles;
            r.slots = plan.slots;
            r.first_slot = c.slot;
            r.in_a_slots = in_a_dev;
            r.in_b_slots = in_b_dev;
            if (sched_dt) {
                r.sched_dt = sched_dt + c.first_cycle;
                r.sched_model = sched_model + c.first_cycle;
            }
        } else {
            const size_t s = size_t(c.slot) * size_t(e->cap);
            if (in_a_dev) e->in_a_bound = static_cast<const char*>(in_a_dev) + s * 3 * w;
            if (in_b_dev) e->in_b_bound = static_cast<const char*>(in_b_dev) + s * 3 * w;
            r.do_update = !sched_model || sched_model[c.first_cycle] >= 0;
            r.dt_uniform = sched_dt ? sched_dt[c.first_cycle] : dt;
            r.meas_uniform = sched_model ? sched_model[c.first_cycle] : meas_model;
            r.meas_dev = meas_dev ? meas_dev + s : nullptr;
            r.z_dev = static_cast<const char*>(z_dev) + s * 3 * w;
            r.Q_dev = static_cast<const char*>(Q_dev) + s * 9 * w;
        }
        rc = launch(e, r);
    }
    e->in_a_bound = keep_a;
    e->in_b_bound = keep_b;
    return rc;
}

// meas_dev != NULL: per-filter model ids, a ring [slots][capacity] like z and Q (meas_model is then ignored)
int cycle_multi_impl(ukfb_engine* e, int cycles, double dt, int meas_model, const int32_t* meas_dev, int slots, int first_slot,
                     const void* in_a_dev, const void* in_b_dev, const void* z_dev, const void* Q_dev) {
    if (!e || !z_dev || !Q_dev) return UKFB_ERR_INVALID_ARG;
    const ukfb::Verdict v = ukfb::check_cycle_args(cycles, slots, first_slot);
    if (v.rc) return fail(v.rc, v.msg);
    if (const int rc = meas_dev ? UKFB_OK : check_meas_model(e, meas_model)) return rc;
    const ukfb::CyclePlan plan(cycles, slots, first_slot, e->cfg.lanes_per_filter == 16, false);
    return run_cycle_plan(e, plan, dt, meas_model, nullptr, nullptr, meas_dev, in_a_dev, in_b_dev, z_dev, Q_dev);
}
}  // namespace

extern "C" {

// ---- predict ------------------------------------------------------------------------------------
int ukfb_predict(ukfb_engine* e, double dt) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    ukfb::LaunchReq r;
    r.do_predict = true;
    r.dt_uniform = dt;
    return launch(e, r);
}

int ukfb_predict_dt_dev(ukfb_engine* e, const double* dt_dev) {
    if (!e || !dt_dev) return UKFB_ERR_INVALID_ARG;
    ukfb::LaunchReq r;
    r.do_predict = true;
    r.dt_dev = dt_dev;
    return launch(e, r);
}

int ukfb_predict_dt(ukfb_engine* e, const double* dt) {
    if (!e || !dt) return UKFB_ERR_INVALID_ARG;
    ON_DEVICE(e->device);
    int rc = upload_raw(e, e->dt_stage, dt, size_t(e->cap));
    if (rc) return rc;
    return ukfb_predict_dt_dev(e, e->dt_stage);
}

int ukfb_predict_timestamps_dev(ukfb_engine* e, const int64_t* ts_us_dev) {
    if (!e || !ts_us_dev) return UKFB_ERR_INVALID_ARG;
    ukfb::LaunchReq r;
    r.do_predict = true;
    r.ts_dev = ts_us_dev;
    return launch(e, r);
}

int ukfb_predict_timestamps(ukfb_engine* e, const int64_t* ts_us) {
    if (!e || !ts_us) return UKFB_ERR_INVALID_ARG;
    ON_DEVICE(e->device);
    int rc = upload_raw(e, e->ts_stage, ts_us, size_t(e->cap));
    if (rc) return rc;
    return ukfb_predict_timestamps_dev(e, e->ts_stage);
}

// ---- update -------------------------------------------------------------------------------------
int ukfb_update_dev(ukfb_engine* e, int meas_model_uniform, const int32_t* meas_model_dev, const void* z_dev,
                    const void* Q_dev) {
    if (!e || !z_dev || !Q_dev) return UKFB_ERR_INVALID_ARG;
    if (const int rc = meas_model_dev ? UKFB_OK : check_meas_model(e, meas_model_uniform)) return rc;
    ukfb::LaunchReq r;
    r.do_update = true;
    r.meas_uniform = meas_model_uniform;
    r.meas_dev = meas_model_dev;
    r.z_dev = z_dev;
    r.Q_dev = Q_dev;
    return launch(e, r);
}

int ukfb_update(ukfb_engine* e, int meas_model, const double* z, const double* Q, const uint8_t* active) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (const int rc = check_meas_model(e, meas_model)) return rc;
    ON_DEVICE(e->device);
    ukfb::LaunchReq r;
    r.do_update = true;
    r.meas_uniform = meas_model;
    // the common form: samples uploaded on the copy stream while the previous kernel runs (see launch_staged)
    if (!active) return launch_staged(e, r, z, Q, size_t(e->cap) * 9);
    const int rc = stage_measurements(e, z, Q, nullptr, active);
    if (rc) return rc;
    r.z_dev = e->z_stage;
    r.Q_dev = e->Q_stage;
    r.active_dev = active ? e->active_stage : nullptr;
    return launch(e, r);
}

int ukfb_update_mixed(ukfb_engine* e, const int32_t* meas_model, const double* z, const double* Q) {
    if (!e || !meas_model) return UKFB_ERR_INVALID_ARG;
    ON_DEVICE(e->device);
    int rc = stage_measurements(e, z, Q, meas_model, nullptr);
    if (rc) return rc;
    ukfb::LaunchReq r;
    r.do_update = true;
    r.meas_dev = e->meas_stage;
    r.z_dev = e->z_stage;
    r.Q_dev = e->Q_stage;
    return launch(e, r);
}

// ---- fused cycle --------------------------------------------------------------------------------
int ukfb_cycle_dev(ukfb_engine* e, double dt, int meas_model_uniform, const int32_t* meas_model_dev, const void* z_dev,
                   const void* Q_dev) {
    if (!e || !z_dev || !Q_dev) return UKFB_ERR_INVALID_ARG;
    if (const int rc = meas_model_dev ? UKFB_OK : check_meas_model(e, meas_model_uniform)) return rc;
    ukfb::LaunchReq r;
    r.do_predict = true;
    r.do_update = true;
    r.dt_uniform = dt;
    r.meas_uniform = meas_model_uniform;
    r.meas_dev = meas_model_dev;
    r.z_dev = z_dev;
    r.Q_dev = Q_dev;
    if (ukfb::buckets_apply(meas_model_dev != nullptr, e->cfg, e->cap)) {
        // Mixed stream: wavefronts of four neighbouring filters would each run the most expensive path any of the four
        // needs.  Group the filters by the class of their update first (device side, nothing read back), then ONE indirect
        // launch over the grouped list: every wavefront is class-uniform, the sigma-point branch of the update is taken by
        // the wavefronts of that class only.
        if (const int rc = refuse_poisoned(e)) return rc;
        ON_DEVICE(e->device);
        int64_t items = 0;
        const int rc = build_model_buckets(e, meas_model_dev, &items);
        if (rc) return rc;
        r.filter_index_dev = e->bucket_idx;
        r.inputs_by_filter = true;
        r.n_items = items;
    }
    return launch(e, r);
}

int ukfb_cycle_multi_dev(ukfb_engine* e, int cycles, double dt, int meas_model, int slots, int first_slot,
                         const void* in_a_dev, const void* in_b_dev, const void* z_dev, const void* Q_dev) {
    return cycle_multi_impl(e, cycles, dt, meas_model, nullptr, slots, first_slot, in_a_dev, in_b_dev, z_dev, Q_dev);
}

int ukfb_cycle_multi_mixed_dev(ukfb_engine* e, int cycles, double dt, int slots, int first_slot, const void* in_a_dev,
                               const void* in_b_dev, const int32_t* meas_model_dev, const void* z_dev, const void* Q_dev) {
    if (!meas_model_dev) return UKFB_ERR_INVALID_ARG;
    return cycle_multi_impl(e, cycles, dt, -1, meas_model_dev, slots, first_slot, in_a_dev, in_b_dev, z_dev, Q_dev);
}

int ukfb_cycle_schedule_dev(ukfb_engine* e, int cycles, const double* dt, const int32_t* meas_model, int slots, int first_slot,
                            const void* in_a_dev, const void* in_b_dev, const void* z_dev, const void* Q_dev) {
    if (!e || !dt || !meas_model || !z_dev || !Q_dev) return UKFB_ERR_INVALID_ARG;
    const ukfb::Verdict v = ukfb::check_cycle_args(cycles, slots, first_slot);
    if (v.rc) return fail(v.rc, v.msg);
    for (int c = 0; c < cycles; ++c)
        if (const int rc = meas_model[c] >= 0 ? check_meas_model(e, meas_model[c]) : UKFB_OK) return rc;
    const ukfb::CyclePlan plan(cycles, slots, first_slot, e->cfg.lanes_per_filter == 16, true);
    return run_cycle_plan(e, plan, 0.0, -1, dt, meas_model, nullptr, in_a_dev, in_b_dev, z_dev, Q_dev);
}

int ukfb_cycle_multi(ukfb_engine* e, int cycles, double dt, int meas_model, const double* in_a, const double* in_b,
                     const double* z, const double* Q) {
    if (!e || !z || !Q) return UKFB_ERR_INVALID_ARG;
    if (cycles < 0) return fail(UKFB_ERR_INVALID_ARG, "cycles >= 0");
    if (const int rc = check_meas_model(e, meas_model)) return rc;
    if (cycles == 0) return UKFB_OK;
    ON_DEVICE(e->device);
    // device rings of this call's samples, one slot per cycle: [z | Q | in_a | in_b]
    const size_t per = size_t(cycles) * size_t(e->cap);
    const size_t nz = per * 3, nq = per * 9, na = in_a ? per * 3 : 0, nb = in_b ? per * 3 : 0;
    const size_t bytes = (nz + nq + na + nb) * e->tsize;
    if (e->multi_bytes < bytes) {
        ENGINE_SYNC(e);
        if (e->multi_dev) HIP_TRY(hipFree(e->multi_dev));
        e->multi_dev = nullptr;
        e->multi_bytes = 0;
        HIP_TRY(hipMalloc(&e->multi_dev, bytes));
        e->multi_bytes = bytes;
    }
    char* base = static_cast<char*>(e->multi_dev);
    void* z_dev = base;
    void* Q_dev = base + nz * e->tsize;
    void* a_dev = in_a ? base + (nz + nq) * e->tsize : nullptr;
    void* b_dev = in_b ? base + (nz + nq + na) * e->tsize : nullptr;
    int rc = upload(e, z_dev, 0, z, nz);
    if (!rc) rc = upload(e, Q_dev, 0, Q, nq);
    if (!rc && in_a) rc = upload(e, a_dev, 0, in_a, na);
    if (!rc && in_b) rc = upload(e, b_dev, 0, in_b, nb);
    if (rc) return rc;
    return ukfb_cycle_multi_dev(e, cycles, dt, meas_model, cycles, 0, a_dev, b_dev, z_dev, Q_dev);
}

// ---- batch-uniform measurement covariance -------------------------------------------------------
int ukfb_cycle_uniform_q_dev(ukfb_engine* e, double dt, int meas_model, const void* z_dev, const void* Q9_dev) {
    if (!e || !z_dev || !Q9_dev) return UKFB_ERR_INVALID_ARG;
    if (const int rc = check_meas_model(e, meas_model)) return rc;
    ukfb::LaunchReq r;
    r.do_predict = true;
    r.do_update = true;
    r.dt_uniform = dt;
    r.meas_uniform = meas_model;
    r.z_dev = z_dev;
    r.Q_dev = Q9_dev;
    r.q_uniform = true;
    return launch(e, r);
}

int ukfb_cycle_uniform_q(ukfb_engine* e, double dt, int meas_model, const double* z, const double* Q9) {
    if (!e || !z || !Q9) return UKFB_ERR_INVALID_ARG;
    if (const int rc = check_meas_model(e, meas_model)) return rc;
    ON_DEVICE(e->device);
    ukfb::LaunchReq r;
    r.do_predict = true;
    r.do_update = true;
    r.dt_uniform = dt;
    r.meas_uniform = meas_model;
    r.q_uniform = true;
    return launch_staged(e, r, z, Q9, 9);
}

int ukfb_update_uniform_q(ukfb_engine* e, int meas_model, const double* z, const double* Q9, const uint8_t* active) {
    if (!e || !z || !Q9) return UKFB_ERR_INVALID_ARG;
    if (const int rc = check_meas_model(e, meas_model)) return rc;
    ON_DEVICE(e->device);
    int rc = upload(e, e->z_stage, 0, z, size_t(e->cap) * 3);
    if (!rc) rc = upload(e, e->Q_stage, 0, Q9, 9);
    if (!rc && active) rc = upload_raw(e, e->active_stage, active, size_t(e->cap));
    if (rc) return rc;
    ukfb::LaunchReq r;
    r.do_update = true;
    r.meas_uniform = meas_model;
    r.z_dev = e->z_stage;
    r.Q_dev = e->Q_stage;
    r.q_uniform = true;
    r.active_dev = active ? e->active_stage : nullptr;
    return launch(e, r);
}

int ukfb_cycle(ukfb_engine* e, double dt, int meas_model, const double* z, const double* Q) {
    if (!e) return UKFB_ERR_INVALID_ARG;
    if (const int rc = check_meas_model(e, meas_model)) return rc;
    ON_DEVICE(e->device);
    ukfb::LaunchReq r;
    r.do_predict = true;
    r.do_update = true;
    r.dt_uniform = dt;
    r.meas_uniform = meas_model;
    return launch_staged(e, r, z, Q, size_t(e->cap) * 9);
}

int ukfb_cycle_timestamps_dev(ukfb_engine* e, const int64_t* ts_us_dev, const int32_t* meas_model_dev, const void* z_dev,
                              const void* Q_dev) {
    if (!e || !ts_us_dev || !meas_model_dev || !z_dev || !Q_dev) return UKFB_ERR_INVALID_ARG;
    ukfb::LaunchReq r;
    r.do_predict = true;
    r.do_update = true;
    r.ts_dev = ts_us_dev;
    r.meas_dev = meas_model_dev;
    r.z_dev = z_dev;
    r.Q_dev = Q_dev;
    return launch(e, r);
}

int ukfb_cycle_timestamps(ukfb_engine* e, const int64_t* ts_us, const int32_t* meas_model, const double* z, const double* Q) {
    if (!e || !ts_us || !meas_model) return UKFB_ERR_INVALID_ARG;
    ON_DEVICE(e->device);
    int rc = stage_measurements(e, z, Q, meas_model, nullptr);
    if (rc) return rc;
    rc = upload_raw(e, e->ts_stage, ts_us, size_t(e->cap));
    if (rc) return rc;
    return ukfb_cycle_timestamps_dev(e, e->ts_stage, e->meas_stage, e->z_stage, e->Q_stage);
}

}  // extern "C"
