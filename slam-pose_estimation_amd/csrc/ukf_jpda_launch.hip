// ukf_jpda_launch.hip -- typed launch of ukf_jpda_kernel<TS>: one instantiation per engine precision (the solve is fp64 in
// both), on the geometry ukf_host.hpp states.  The rule's three logarithms are formed in double and rounded to the engine's
// storage type, as the PDA launch rounds them.
#include "ukf_api_common.hpp"
#include "ukf_jpda.hpp"

namespace ukfb {

namespace {

template <class TS> int run(ukfb_engine* e, const ukfb_jpda_in& in, const ukfb_pda_rule& rule, const ukfb_jpda_out& out) {
    const JpdaGeometry geo = jpda_geometry(in.scenes);
    JpdaArgs<TS> a{};
    a.loglik = static_cast<const TS*>(in.loglik_dev);
    a.maha = static_cast<const TS*>(in.maha_dev);
    a.model = in.model_dev;
    a.scene_start = in.scene_start_dev;
    a.beta = static_cast<TS*>(out.beta);
    a.beta0 = static_cast<TS*>(out.beta0);
    a.free_k = out.free;
    a.log_z = out.log_z;
    a.scene_status = out.scene_status;
    a.gate = in.gate;
    const PdaLogs lg = pda_logs(rule);   // formed in double
    a.ln_pd = double(TS(lg.ln_pd));
    a.a0_m1 = double(TS(lg.a0_m1));
    a.a0_m3 = double(TS(lg.a0_m3));
    a.cap = e->cap;
    a.scenes = in.scenes;
    a.K = in.candidates;
    a.tracks_per_scene = in.tracks_per_scene;
    a.model_uniform = in.model_uniform;
    a.engine_model = e->model;
    hipLaunchKernelGGL(ukf_jpda_kernel<TS>, dim3(unsigned(geo.grid)), dim3(JPDA_THREADS), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("joint association kernel launch");
}

}  // namespace

int launch_jpda(ukfb_engine* e, const ukfb_jpda_in& in, const ukfb_pda_rule& rule, const ukfb_jpda_out& out) {
    if (in.scenes == 0) return UKFB_OK;
    return e->prec == UKFB_F64 ? run<double>(e, in, rule, out) : run<float>(e, in, rule, out);
}

}  // namespace ukfb
