// ukf_relative_launch.inc.hpp -- typed launch of ukf_relative_kernel<T, M, TS>; included by the Pose translation unit.
// The three instantiations: fp64, fp32, fp32 arrays with fp64 arithmetic (wide_arithmetic).
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_relative.hpp"
#include "ukf_relative_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_relative_typed(ukfb_engine* e, const RelativeReq& r) {
    using MC = typename M::template rebind<TC>;
    constexpr int D = MC::D;
    const RowGeometry geo = relative_geometry(MC::S, D, e->cap, sizeof(TC));
    if (geo.grid == 0) return UKFB_OK;
    RelativeArgs<TC, TS> a{};
    a.n = e->cap;
    a.mu = static_cast<const TS*>(e->mu);
    a.cov = static_cast<const TS*>(e->cov);
    // commit = 0: the kernel gets no pointer through which it could store to the engine
    a.eng_mu = r.commit ? static_cast<TS*>(e->mu) : nullptr;
    a.eng_cov = r.commit ? static_cast<TS*>(e->cov) : nullptr;
    a.engine_status = r.commit ? e->status : nullptr;
    a.mu_hist = static_cast<const TS*>(r.in.mu_hist_dev);
    a.cov_hist = static_cast<const TS*>(r.in.cov_hist_dev);
    a.slots = r.in.slots;
    a.back = r.in.steps - 1;
    a.top_slot = int((int64_t(r.in.first_slot) + a.back) % r.in.slots);
    for (int k = 0; k < a.back && k < SMOOTH_MAX_BACK; ++k) a.dt[k] = r.in.dt[a.back - 1 - k];
    a.initialised = e->init;
    a.Rn = static_cast<const TS*>(e->Rn);
    a.Rn_stride = e->Rn_per_filter ? int64_t(D) * D : 0;
    a.Racc = static_cast<const TS*>(e->Racc);
    a.in_a = static_cast<const TS*>(r.in.in_a_dev ? r.in.in_a_dev : (e->in_a_bound ? e->in_a_bound : e->in_a));
    a.in_b = static_cast<const TS*>(r.in.in_b_dev ? r.in.in_b_dev : (e->in_b_bound ? e->in_b_bound : e->in_b));
    a.in_ring = (r.in.in_a_dev ? 1 : 0) | (r.in.in_b_dev ? 2 : 0);
    a.ninv_tau_g = TC(TS(-1.0) / TS(e->tau_g));   // (rounded as the forward launches round them)
    a.ninv_tau_a = TC(TS(-1.0) / TS(e->tau_a));
    for (int k = 0; k < 3; ++k) a.earth[k] = TC(TS(e->earth[k]));
    a.mean_tol = TC(TS(e->cfg.mean_tol));
    a.mean_max_it = e->cfg.mean_max_iter;
    a.min_dt = e->cfg.min_time_delta;
    a.max_dt = e->cfg.max_time_delta;
    a.lag_uniform = r.in.lag_uniform;
    a.lag = r.in.lag_dev;
    a.model_uniform = r.in.model_uniform;
    a.model = r.in.model_dev;
    a.z = static_cast<const TS*>(r.in.z_dev);
    a.Q = static_cast<const TS*>(r.in.Q_dev);
    a.q_uniform = r.in.q_is_uniform;
    a.gate_chi2 = TC(TS(e->cfg.gate_chi2));
    a.z_pred = static_cast<TS*>(r.out.z_pred);
    a.S = static_cast<TS*>(r.out.S);
    a.innov = static_cast<TS*>(r.out.innov);
    a.maha = static_cast<TS*>(r.out.maha);
    a.loglik = static_cast<TS*>(r.out.loglik);
    a.status = r.out.status;
    a.mu_out = static_cast<TS*>(r.out.mu_out);
    a.cov_out = static_cast<TS*>(r.out.cov_out);
    hipLaunchKernelGGL((ukf_relative_kernel<TC, MC, TS>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("relative-measurement kernel launch");
}

template <class M64, class M32> static int launch_relative_model(ukfb_engine* e, const RelativeReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_relative_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

}  // namespace ukfb
