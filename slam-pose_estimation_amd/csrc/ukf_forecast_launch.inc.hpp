// ukf_forecast_launch.inc.hpp -- typed launch of ukf_forecast_kernel<T, M, TS>; included by the two per-model translation
// units.  The three instantiations of a model: fp64, fp32, fp32 arrays with fp64 arithmetic (wide_arithmetic).
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_forecast.hpp"
#include "ukf_forecast_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_forecast_typed(ukfb_engine* e, const ForecastReq& r) {
    using MC = typename M::template rebind<TC>;
    constexpr int S = MC::S, D = MC::D;
    const RowGeometry geo = forecast_geometry(S, D, e->cap, sizeof(TC));
    if (geo.grid == 0) return UKFB_OK;
    ForecastArgs<TC, TS> a{};
    a.n = e->cap;
    // the engine's state goes in as a pointer to const, like everything else of the engine: the kernel cannot store to it
    a.start_mu = static_cast<const TS*>(r.start_mu_dev ? r.start_mu_dev : static_cast<const void*>(e->mu));
    a.start_cov = static_cast<const TS*>(r.start_cov_dev ? r.start_cov_dev : static_cast<const void*>(e->cov));
    a.mu_out = static_cast<TS*>(r.mu_out_dev);
    a.cov_out = static_cast<TS*>(r.cov_out_dev);
    a.slots = r.slots;
    a.first_slot = r.first_slot;
    a.steps = r.steps;
    a.use_ts = r.ts_us ? 1 : 0;
    for (int k = 0; k < r.steps && k < FORECAST_MAX_STEPS; ++k) {
        if (r.dt) a.dt[k] = r.dt[k];
        if (r.ts_us) a.ts_us[k] = r.ts_us[k];
    }
    a.initialised = e->init;
    a.last_ts = e->last_ts;
    a.Rn = static_cast<const TS*>(e->Rn);
    a.Rn_stride = e->Rn_per_filter ? int64_t(D) * D : 0;
    a.Racc = static_cast<const TS*>(e->Racc);
    a.in_a = static_cast<const TS*>(r.in_a_dev ? r.in_a_dev : (e->in_a_bound ? e->in_a_bound : e->in_a));
    a.in_b = static_cast<const TS*>(r.in_b_dev ? r.in_b_dev : (e->in_b_bound ? e->in_b_bound : e->in_b));
    a.in_ring = (r.in_a_dev ? 1 : 0) | (r.in_b_dev ? 2 : 0);
    a.ninv_tau_g = TC(TS(-1.0) / TS(e->tau_g));   // (rounded as the forward launches round them)
    a.ninv_tau_a = TC(TS(-1.0) / TS(e->tau_a));
    for (int k = 0; k < 3; ++k) a.earth[k] = TC(TS(e->earth[k]));
    a.mean_tol = TC(TS(e->cfg.mean_tol));
    a.mean_max_it = e->cfg.mean_max_iter;
    a.min_dt = e->cfg.min_time_delta;
    a.max_dt = e->cfg.max_time_delta;
    a.status = r.status_dev;
    hipLaunchKernelGGL((ukf_forecast_kernel<TC, MC, TS>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("forecast kernel launch");
}

template <class M64, class M32> static int launch_forecast_model(ukfb_engine* e, const ForecastReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_forecast_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

}  // namespace ukfb
