// ukf_assign_launch.hip -- typed launch of ukf_assign_kernel<TS>: one instantiation per engine precision (the solve is fp64 in
// both, and knows nothing of the engine's model), on the geometry ukf_host.hpp states
#include "ukf_api_common.hpp"
#include "ukf_assign.hpp"

namespace ukfb {

namespace {

template <class TS> int run(ukfb_engine* e, const ukfb_assign_in& in, const ukfb_assign_out& out) {
    const AssignGeometry geo = assign_geometry(in.scenes);
    AssignArgs<TS> a{};
    a.cost = static_cast<const TS*>(in.cost_dev);
    a.miss = static_cast<const TS*>(in.miss_dev);
    a.scene_start = in.scene_start_dev;
    a.assign = out.assign;
    a.owner = out.owner;
    a.objective = out.objective;
    a.scene_status = out.scene_status;
    a.gate = in.gate;
    a.miss_uniform = in.miss_uniform;
    a.cap = e->cap;
    a.scenes = in.scenes;
    a.K = in.candidates;
    a.tracks_per_scene = in.tracks_per_scene;
    hipLaunchKernelGGL(ukf_assign_kernel<TS>, dim3(unsigned(geo.grid)), dim3(ASSIGN_THREADS), 0, main_stream(e), a);
    return launch_status("assignment kernel launch");
}

}  // namespace

int launch_assign(ukfb_engine* e, const ukfb_assign_in& in, const ukfb_assign_out& out) {
    if (in.scenes == 0) return UKFB_OK;
    return e->prec == UKFB_F64 ? run<double>(e, in, out) : run<float>(e, in, out);
}

}  // namespace ukfb
