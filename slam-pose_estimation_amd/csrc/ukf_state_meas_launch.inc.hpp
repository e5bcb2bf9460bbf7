// ukf_state_meas_launch.inc.hpp -- typed launch of ukf_state_meas_kernel<T, M, TS>; included by the two per-model translation
// units.  The three instantiations of a model: fp64, fp32, fp32 arrays with fp64 arithmetic (wide_arithmetic).
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_state_meas.hpp"
#include "ukf_state_meas_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_state_meas_typed(ukfb_engine* e, const StateMeasReq& r) {
    using MC = typename M::template rebind<TC>;
    const RowGeometry geo = state_meas_geometry(MC::S, MC::D, e->cap, sizeof(TC));
    if (geo.grid == 0) return UKFB_OK;
    StateMeasArgs<TC, TS> a{};
    a.n = e->cap;
    a.mu = static_cast<const TS*>(e->mu);
    a.cov = static_cast<const TS*>(e->cov);
    // commit = 0: the kernel gets no pointer through which it could store to the engine
    a.mu_out = r.commit ? static_cast<TS*>(e->mu) : nullptr;
    a.cov_out = r.commit ? static_cast<TS*>(e->cov) : nullptr;
    a.engine_status = r.commit ? e->status : nullptr;
    a.initialised = e->init;
    a.mask_uniform = r.mask_uniform;
    a.mask = r.mask_dev;
    a.z = static_cast<const TS*>(r.z_dev);
    a.Qz = static_cast<const TS*>(r.Qz_dev);
    a.infl_state = TC(r.state_inflation);
    a.infl_meas = TC(r.meas_inflation);
    a.mean_tol = TC(TS(e->cfg.mean_tol));   // (rounded as the forward launches round them)
    a.mean_max_it = e->cfg.mean_max_iter;
    a.gate_chi2 = TC(TS(e->cfg.gate_chi2));
    a.maha = static_cast<TS*>(r.out.maha);
    a.loglik = static_cast<TS*>(r.out.loglik);
    a.status = r.out.status;
    hipLaunchKernelGGL((ukf_state_meas_kernel<TC, MC, TS>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("state-measurement kernel launch");
}

template <class M64, class M32> static int launch_state_meas_model(ukfb_engine* e, const StateMeasReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_state_meas_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

}  // namespace ukfb
