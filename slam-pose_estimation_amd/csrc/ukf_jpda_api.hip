// ukf_jpda_api.hip -- C-ABI of the joint association marginals of a scene (include/ukf_batch_jpda.h): argument checks
// (ukf_host.hpp), the device form and the host-array form.
#include "ukf_api_common.hpp"

extern "C" {

int ukfb_jpda_scenes_dev(ukfb_engine* e, const ukfb_jpda_in* in, const ukfb_pda_rule* rule, const ukfb_jpda_out* out) {
    if (const int rc = ukfb::entry(e)) return rc;
    if (const int rc = ukfb::fail(ukfb::check_jpda_args(e->cap, in, rule, out))) return rc;
    ON_DEVICE(e->device);
    return ukfb::launch_jpda(e, *in, *rule, *out);
}

int ukfb_jpda_scenes(ukfb_engine* e, int candidates, const double* loglik, const double* maha, int scenes, const int32_t* scene_start,
                     int tracks_per_scene, double gate, int model, const int32_t* model_per_filter, const ukfb_pda_rule* rule,
                     double* beta, double* beta0, double* free, double* log_z, uint32_t* scene_status) {
    if (const int rc = ukfb::entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_jpda_in in{};
    in.loglik_dev = loglik;
    in.maha_dev = maha;
    in.candidates = candidates;
    in.scenes = scenes;
    in.scene_start_dev = scene_start;
    in.tracks_per_scene = tracks_per_scene;
    in.gate = gate;
    in.model_uniform = model;
    in.model_dev = model_per_filter;
    const ukfb_jpda_out wanted{beta, beta0, free, log_z, scene_status};
    if (const int rc = ukfb::fail(ukfb::check_jpda_args(e->cap, &in, rule, &wanted))) return rc;
    if (scene_start)
        if (const int rc = ukfb::fail(ukfb::check_assign_offsets(e->cap, scenes, scene_start))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap), ns = size_t(scenes), nk = size_t(candidates) * n;
    ukfb::HostStage stage(e);
    in.loglik_dev = stage.in(loglik, nk);
    in.maha_dev = stage.in(maha, nk);
    in.scene_start_dev = stage.raw_in(scene_start, ns + 1);
    in.model_dev = stage.raw_in(model_per_filter, n);
    ukfb_jpda_out out{};
    out.beta = stage.out(beta, nk);
    out.beta0 = stage.out(beta0, n);
    out.free = stage.raw_out(free, ns * size_t(candidates));
    out.log_z = stage.raw_out(log_z, ns);
    out.scene_status = stage.raw_out(scene_status, ns);
    if (const int rc = stage.rc()) return rc;
    // what the launch does not write reads NaN (all bits set, in either precision): slots no scene covers, too-large scenes
    if (out.beta) HIP_TRY(hipMemsetAsync(out.beta, 0xff, nk * e->tsize, ukfb::main_stream(e)));
    if (out.beta0) HIP_TRY(hipMemsetAsync(out.beta0, 0xff, n * e->tsize, ukfb::main_stream(e)));
    if (out.free) HIP_TRY(hipMemsetAsync(out.free, 0xff, ns * size_t(candidates) * sizeof(double), ukfb::main_stream(e)));
    if (out.log_z) HIP_TRY(hipMemsetAsync(out.log_z, 0xff, ns * sizeof(double), ukfb::main_stream(e)));
    if (const int rc = ukfb_jpda_scenes_dev(e, &in, rule, &out)) return rc;
    return stage.finish();
}

}  // extern "C"
