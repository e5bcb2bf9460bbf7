// ukf_sampled_launch.inc.hpp -- typed launches of ukf_sigma_points_kernel / ukf_sampled_kernel<T, M, TS>; included by the two
// per-model translation units.  The three instantiations of a model: fp64, fp32, fp32 arrays with fp64 arithmetic
// (wide_arithmetic).
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_sampled.hpp"
#include "ukf_sampled_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_sigma_points_typed(ukfb_engine* e, const SigmaPointsReq& r) {
    using MC = typename M::template rebind<TC>;
    const RowGeometry geo = sigma_points_geometry(MC::S, MC::D, e->cap, sizeof(TC));
    if (geo.grid == 0) return UKFB_OK;
    SigmaPointsArgs<TC, TS> a{};
    a.n = e->cap;
    a.mu = static_cast<const TS*>(e->mu);
    a.cov = static_cast<const TS*>(e->cov);
    a.initialised = e->init;
    a.X = static_cast<TS*>(r.X);
    a.delta = static_cast<TS*>(r.delta);
    a.status = r.status;
    hipLaunchKernelGGL((ukf_sigma_points_kernel<TC, MC, TS>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("sigma-point export kernel launch");
}

template <class TS, class M, class TC> static int launch_sampled_typed(ukfb_engine* e, const SampledReq& r) {
    using MC = typename M::template rebind<TC>;
    const RowGeometry geo = sampled_geometry(MC::S, MC::D, e->cap, sizeof(TC));
    if (geo.grid == 0) return UKFB_OK;
    SampledArgs<TC, TS> a{};
    a.n = e->cap;
    a.mu = static_cast<const TS*>(e->mu);
    a.cov = static_cast<const TS*>(e->cov);
    // commit = 0: the kernel gets no pointer through which it could store to the engine
    a.mu_out = r.commit ? static_cast<TS*>(e->mu) : nullptr;
    a.cov_out = r.commit ? static_cast<TS*>(e->cov) : nullptr;
    a.engine_status = r.commit ? e->status : nullptr;
    a.initialised = e->init;
    a.m = r.in.m;
    a.Z = static_cast<const TS*>(r.in.Z_dev);
    a.z = static_cast<const TS*>(r.in.z_dev);
    a.Q = static_cast<const TS*>(r.in.Q_dev);
    a.q_uniform = r.in.q_is_uniform;
    a.active = r.in.active_dev;
    a.mean_tol = TC(TS(e->cfg.mean_tol));   // (rounded as the forward launches round them)
    a.mean_max_it = e->cfg.mean_max_iter;
    a.gate_chi2 = TC(TS(e->cfg.gate_chi2));
    a.z_pred = static_cast<TS*>(r.out.z_pred);
    a.S = static_cast<TS*>(r.out.S);
    a.innov = static_cast<TS*>(r.out.innov);
    a.maha = static_cast<TS*>(r.out.maha);
    a.loglik = static_cast<TS*>(r.out.loglik);
    a.status = r.out.status;
    hipLaunchKernelGGL((ukf_sampled_kernel<TC, MC, TS>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("sampled-update kernel launch");
}

template <class M64, class M32> static int launch_sigma_points_model(ukfb_engine* e, const SigmaPointsReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_sigma_points_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

template <class M64, class M32> static int launch_sampled_model(ukfb_engine* e, const SampledReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_sampled_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

}  // namespace ukfb
