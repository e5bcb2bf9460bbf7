// ukf_associate_launch.inc.hpp -- typed launch of ukf_associate_kernel<T, M, TS, HYP>; included by the two per-model
// translation units.  The three instantiations of a model (fp64, fp32, fp32 arrays with fp64 arithmetic), each in the
// shared-h and the per-hypothesis mode.
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_associate.hpp"
#include "ukf_associate_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_associate_typed(ukfb_engine* e, const AssociateReq& r) {
    using MC = typename M::template rebind<TC>;
    const RowGeometry geo = sensor_geometry(MC::S, MC::D, e->cap, sizeof(TC));   // the sensor kernel's LDS map
    if (geo.grid == 0) return UKFB_OK;
    AssociateArgs<TC, TS> a{};
    a.n = e->cap;
    a.mu = static_cast<const TS*>(e->mu);
    a.cov = static_cast<const TS*>(e->cov);
    // commit = 0: the kernel gets no pointer through which it could store to the engine
    a.mu_out = r.commit ? static_cast<TS*>(e->mu) : nullptr;
    a.cov_out = r.commit ? static_cast<TS*>(e->cov) : nullptr;
    a.engine_status = r.commit ? e->status : nullptr;
    a.initialised = e->init;
    a.model_uniform = r.model_uniform;
    a.model = r.in.model_dev;
    a.candidates = r.in.candidates;
    a.z = static_cast<const TS*>(r.in.z_dev);
    a.Q = static_cast<const TS*>(r.in.Q_dev);
    a.q_uniform = r.in.q_is_uniform;
    a.mount = static_cast<const TS*>(r.in.mount_dev);
    a.point = static_cast<const TS*>(r.in.point_dev);
    // (rounded to the engine's storage first: the value a per-filter array would hold)
    for (int k = 0; k < 7; ++k) a.mount_u[k] = TC(TS(r.in.mount_uniform[k]));
    for (int k = 0; k < 3; ++k) a.point_u[k] = TC(TS(r.in.point_uniform[k]));
    a.gyro = static_cast<const TS*>(e->in_b_bound ? e->in_b_bound : e->in_b);
    a.mean_tol = TC(TS(e->cfg.mean_tol));   // (rounded as the forward launches round them)
    a.mean_max_it = e->cfg.mean_max_iter;
    a.gate_chi2 = TC(TS(e->cfg.gate_chi2));
    a.z_pred = static_cast<TS*>(r.out.z_pred);
    a.S = static_cast<TS*>(r.out.S);
    a.innov = static_cast<TS*>(r.out.innov);
    a.maha = static_cast<TS*>(r.out.maha);
    a.loglik = static_cast<TS*>(r.out.loglik);
    a.best = r.out.best;
    a.n_gated = r.out.n_gated;
    a.status = r.out.status;
    if (r.in.point_per_candidate)
        hipLaunchKernelGGL((ukf_associate_kernel<TC, MC, TS, true>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    else
        hipLaunchKernelGGL((ukf_associate_kernel<TC, MC, TS, false>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("sensor-association kernel launch");
}

template <class M64, class M32> static int launch_associate_model(ukfb_engine* e, const AssociateReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_associate_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

}  // namespace ukfb
