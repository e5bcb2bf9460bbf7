// ukf_assign_api.hip -- C-ABI of the assignment across the filters of a scene (include/ukf_batch_assign.h): argument checks
// (ukf_host.hpp), the device form and the host-array form.
#include "ukf_api_common.hpp"

extern "C" {

int ukfb_assign_scenes_dev(ukfb_engine* e, const ukfb_assign_in* in, const ukfb_assign_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_assign_args(e->cap, in, out))) return rc;
    ON_DEVICE(e->device);
    return ukfb::launch_assign(e, *in, *out);
}

int ukfb_assign_scenes(ukfb_engine* e, int candidates, const double* cost, int scenes, const int32_t* scene_start,
                       int tracks_per_scene, double gate, const double* miss, double miss_uniform, int32_t* assign, int32_t* owner,
                       double* objective, uint32_t* scene_status) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_assign_in in{};
    in.cost_dev = cost;
    in.candidates = candidates;
    in.scenes = scenes;
    in.scene_start_dev = scene_start;
    in.tracks_per_scene = tracks_per_scene;
    in.gate = gate;
    in.miss_dev = miss;
    in.miss_uniform = miss_uniform;
    const ukfb_assign_out wanted{assign, owner, objective, scene_status};
    if (const int rc = ukfb::fail(ukfb::check_assign_args(e->cap, &in, &wanted))) return rc;
    if (scene_start)
        if (const int rc = ukfb::fail(ukfb::check_assign_offsets(e->cap, scenes, scene_start))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), ns = size_t(scenes), nk = ns * size_t(candidates);
    ukfb::HostStage stage(e);
    in.cost_dev = stage.in(cost, size_t(candidates) * n);
    in.scene_start_dev = stage.raw_in(scene_start, ns + 1);
    in.miss_dev = stage.in(miss, n);
    ukfb_assign_out out{};
    out.assign = stage.raw_out(assign, n);
    out.owner = stage.raw_out(owner, nk);
    out.objective = stage.raw_out(objective, ns);
    out.scene_status = stage.raw_out(scene_status, ns);
    if (const int rc = stage.rc()) return rc;
    // slots no scene covers are not written by the launch: they read -1
    if (out.assign) HIP_TRY(hipMemsetAsync(out.assign, 0xff, n * sizeof(int32_t), ukfb::main_stream(e)));
    if (const int rc = ukfb_assign_scenes_dev(e, &in, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
