// ukf_innovation_launch.inc.hpp -- typed launch of ukf_innovation_kernel<T, M, TS>; included by the two per-model
// translation units.  The three instantiations of a model: fp64, fp32, fp32 arrays with fp64 arithmetic (wide_arithmetic).
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_innovation.hpp"
#include "ukf_innovation_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_innovation_typed(ukfb_engine* e, const InnovReq& r) {
    using MC = typename M::template rebind<TC>;
    InnovArgs<TS> a{};
    a.n = e->cap;
    a.mu = static_cast<const TS*>(e->mu);
    a.cov = static_cast<const TS*>(e->cov);
    a.initialised = e->init;
    a.meas_uniform = r.meas_uniform;
    a.meas = r.meas_dev;
    a.candidates = r.candidates;
    a.z = static_cast<const TS*>(r.z_dev);
    a.Q = static_cast<const TS*>(r.Q_dev);
    a.q_uniform = r.q_uniform ? 1 : 0;
    a.mean_tol = TS(e->cfg.mean_tol);
    a.mean_max_it = e->cfg.mean_max_iter;
    a.gate_chi2 = TS(e->cfg.gate_chi2);
    a.z_pred = static_cast<TS*>(r.out.z_pred);
    a.S = static_cast<TS*>(r.out.S);
    a.innov = static_cast<TS*>(r.out.innov);
    a.maha = static_cast<TS*>(r.out.maha);
    a.loglik = static_cast<TS*>(r.out.loglik);
    a.best = r.out.best;
    a.status = r.out.status;
    const int64_t grid = (a.n + 3) / 4;
    if (grid == 0) return UKFB_OK;
    hipLaunchKernelGGL((ukf_innovation_kernel<TC, MC, TS>), dim3((unsigned)grid), dim3(64), 0, main_stream(e), a);
    return launch_status("innovation kernel launch");
}

template <class M64, class M32> static int launch_innovation_model(ukfb_engine* e, const InnovReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_innovation_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

}  // namespace ukfb
