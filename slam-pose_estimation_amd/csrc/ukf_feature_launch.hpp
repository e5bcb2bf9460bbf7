// ukf_feature_launch.hpp -- the launch layer of the feature kernels, between the C ABI (ukf_<feature>_api.hip, which calls
// launch_for_model, ukf_feature_bind.hpp) and a kernel header.  A feature's ukf_<feature>_launch.hip states its typed launch
// once, as FeatureLaunch<Req>::run<TS, MC, TC>: it fills the argument struct (the engine's part through the binders) and ends
// in launch_rows.  The choice of the instantiation by precision and model, and the launch itself, are here.
#pragma once

#include "ukf_feature_bind.hpp"
#include "ukf_device.hpp"

namespace ukfb {

// template <class TS, class MC, class TC> static int run(ukfb_engine*, const Req&): storage type, model over the compute type,
// compute type
template <class Req> struct FeatureLaunch;

// The tail of every typed launch: nothing for an empty grid, else one wavefront per workgroup on the engine's stream with the
// LDS bytes of the geometry (RowGeometry, BankGeometry).
template <class A, class Geo> int launch_rows(ukfb_engine* e, void (*kernel)(A), const Geo& geo, const char* what, const A& a) {
    if (geo.grid == 0) return UKFB_OK;
    hipLaunchKernelGGL(kernel, dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status(what);
}

template <class M64, class M32, class Req> int launch_model(ukfb_engine* e, const Req& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return FeatureLaunch<Req>::template run<typename P::TS, typename P::M::template rebind<typename P::TC>, typename P::TC>(e, r);
    });
}

template <class Req> int launch_pose(ukfb_engine* e, const Req& r) { return launch_model<PoseM<double>, PoseM<float>>(e, r); }
template <class Req> int launch_orient(ukfb_engine* e, const Req& r) { return launch_model<OrientM<double>, OrientM<float>>(e, r); }

}  // namespace ukfb

// A launch source is compiled once per model (csrc/Makefile: -DUKFB_LAUNCH_POSE / -DUKFB_LAUNCH_ORIENT name the model of the
// object), so that a model's kernels are built in parallel and by themselves.  UKFB_LAUNCH_UNIT(Req), at the end of the source
// inside namespace ukfb, instantiates the launch of that model.
#if defined(UKFB_LAUNCH_POSE) == defined(UKFB_LAUNCH_ORIENT)
#error "a feature launch source is compiled with exactly one of -DUKFB_LAUNCH_POSE and -DUKFB_LAUNCH_ORIENT"
#elif defined(UKFB_LAUNCH_POSE)
#define UKFB_LAUNCH_UNIT(Req) template int launch_pose<Req>(ukfb_engine*, const Req&);
#else
#define UKFB_LAUNCH_UNIT(Req) template int launch_orient<Req>(ukfb_engine*, const Req&);
#endif
