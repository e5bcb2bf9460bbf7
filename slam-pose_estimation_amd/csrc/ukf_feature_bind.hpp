// ukf_feature_bind.hpp -- the host half of a feature launch that no feature owns: the choice of instantiation by the engine's
// precision and model, and the binders that fill in what the ENGINE contributes to a kernel's argument struct (state and commit
// pointers, the process model, the mean-iteration and gate scalars, the sensor-frame inputs).  Two contracts live here, once:
//  * rounding -- every scalar reaches the kernel as TC(TS(x)): rounded to the engine's storage type first, the value a forward
//    launch or a per-filter array would hold, then widened to the compute type (the parity tests rest on it);
//  * commit -- a call with commit = 0 gets no pointer through which its kernel could store to the engine.
// The binders are templates over the argument type and name its members, so the layout of every *Args struct stays its
// kernel header's.  No kernel code and no HIP runtime call: tests/cpp/feature_launch_host.cpp runs this header on the CPU.
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

// storage type, model at the compute type's precision class, compute type
template <class TS_, class M_, class TC_> struct Precision {
    using TS = TS_;
    using M = M_;
    using TC = TC_;
};

// f(Precision<...>{}) for the engine's mode: fp64, fp32 arrays with fp64 arithmetic (wide_arithmetic), fp32
template <class M64, class M32, class F> static int dispatch_precision(const ukfb_engine* e, F&& f) {
    if (e->prec == UKFB_F64) return f(Precision<double, M64, double>{});
    if (e->cfg.wide_arithmetic) return f(Precision<float, M32, double>{});
    return f(Precision<float, M32, float>{});
}

// The launch of a request type for one model, at the engine's precision.  ukf_feature_launch.hpp defines both from the
// feature's FeatureLaunch<Req>; the feature's translation units instantiate them.
template <class Req> int launch_pose(ukfb_engine* e, const Req& r);
template <class Req> int launch_orient(ukfb_engine* e, const Req& r);

// true for the request of a feature that has PoseWithVelocity kernels only (its argument check has refused the other model)
template <class Req> inline constexpr bool pose_only = false;

template <class Req> int launch_for_model(ukfb_engine* e, const Req& r) {
    if constexpr (pose_only<Req>)
        return launch_pose(e, r);
    else
        return e->model == UKFB_MODEL_POSE ? launch_pose(e, r) : launch_orient(e, r);
}

// a.engine_status and the two given members: the engine's arrays for a committing call, null otherwise
template <class TS, class A> void bind_commit(A& a, const ukfb_engine* e, bool commit, TS*& mu_store, TS*& cov_store) {
    // commit = 0: the kernel gets no pointer through which it could store to the engine
    mu_store = commit ? static_cast<TS*>(e->mu) : nullptr;
    cov_store = commit ? static_cast<TS*>(e->cov) : nullptr;
    a.engine_status = commit ? e->status : nullptr;
}
template <class TS, class A> void bind_commit(A& a, const ukfb_engine* e, bool commit) { bind_commit<TS>(a, e, commit, a.mu_out, a.cov_out); }

// n, the engine's state to read, and bind_commit; the first form for a struct whose mu_out / cov_out are the caller's outputs
template <class TS, class A> void bind_state(A& a, const ukfb_engine* e, bool commit, TS*& mu_store, TS*& cov_store) {
    a.n = e->cap;
    a.mu = static_cast<const TS*>(e->mu);
    a.cov = static_cast<const TS*>(e->cov);
    a.initialised = e->init;
    bind_commit<TS>(a, e, commit, mu_store, cov_store);
}
template <class TS, class A> void bind_state(A& a, const ukfb_engine* e, bool commit) { bind_state<TS>(a, e, commit, a.mu_out, a.cov_out); }

template <class TS, class TC, class A> void bind_mean(A& a, const ukfb_engine* e) {
    a.mean_tol = TC(TS(e->cfg.mean_tol));
    a.mean_max_it = e->cfg.mean_max_iter;
}

template <class TS, class TC, class A> void bind_gate(A& a, const ukfb_engine* e) { a.gate_chi2 = TC(TS(e->cfg.gate_chi2)); }

// The process model of a kernel that predicts: noise, inputs (the request's ring before a bound array before the latched one),
// time constants, earth rate, the mean iteration and the limits of a time step.  D: the model's tangent dimension.
template <class TS, class TC, class A> void bind_process(A& a, const ukfb_engine* e, int D, const void* in_a_ring, const void* in_b_ring) {
    a.Rn = static_cast<const TS*>(e->Rn);
    a.Rn_stride = e->Rn_per_filter ? int64_t(D) * D : 0;
    a.Racc = static_cast<const TS*>(e->Racc);
    a.in_a = static_cast<const TS*>(in_a_ring ? in_a_ring : (e->in_a_bound ? e->in_a_bound : e->in_a));
    a.in_b = static_cast<const TS*>(in_b_ring ? in_b_ring : (e->in_b_bound ? e->in_b_bound : e->in_b));
    a.in_ring = (in_a_ring ? 1 : 0) | (in_b_ring ? 2 : 0);
    a.ninv_tau_g = TC(TS(-1.0) / TS(e->tau_g));
    a.ninv_tau_a = TC(TS(-1.0) / TS(e->tau_a));
    for (int k = 0; k < 3; ++k) a.earth[k] = TC(TS(e->earth[k]));
    bind_mean<TS, TC>(a, e);
    a.min_dt = e->cfg.min_time_delta;
    a.max_dt = e->cfg.max_time_delta;
}

// What a sensor-frame request (model_uniform, in, out: sensor measurements, bearings, association) gives its kernel.  gyro: the
// bound rotation rate before the latched one, or null for a kernel none of whose models reads it.
template <class TS, class TC, class A, class Req> void bind_sensor_inputs(A& a, const ukfb_engine* e, const Req& r, bool gyro) {
    a.model_uniform = r.model_uniform;
    a.model = r.in.model_dev;
    a.z = static_cast<const TS*>(r.in.z_dev);
    a.Q = static_cast<const TS*>(r.in.Q_dev);
    a.q_uniform = r.in.q_is_uniform;
    a.mount = static_cast<const TS*>(r.in.mount_dev);
    a.point = static_cast<const TS*>(r.in.point_dev);
    for (int k = 0; k < 7; ++k) a.mount_u[k] = TC(TS(r.in.mount_uniform[k]));
    for (int k = 0; k < 3; ++k) a.point_u[k] = TC(TS(r.in.point_uniform[k]));
    a.gyro = gyro ? static_cast<const TS*>(e->in_b_bound ? e->in_b_bound : e->in_b) : nullptr;
    a.z_pred = static_cast<TS*>(r.out.z_pred);
    a.S = static_cast<TS*>(r.out.S);
    a.innov = static_cast<TS*>(r.out.innov);
    a.maha = static_cast<TS*>(r.out.maha);
    a.loglik = static_cast<TS*>(r.out.loglik);
    a.status = r.out.status;
}

}  // namespace ukfb
