// ukf_smooth_launch.inc.hpp -- typed launch of ukf_smooth_kernel<T, M, TS>; included by the two per-model translation units.
// The three instantiations of a model: fp64, fp32, fp32 arrays with fp64 arithmetic (wide_arithmetic).
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_smooth.hpp"
#include "ukf_smooth_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_smooth_typed(ukfb_engine* e, const SmoothReq& r) {
    using MC = typename M::template rebind<TC>;
    constexpr int S = MC::S, D = MC::D, PK = D * (D + 1) / 2;
    const RowGeometry geo = smooth_geometry(S, D, e->cap, sizeof(TC));
    if (geo.grid == 0) return UKFB_OK;
    const SmoothLaunch& p = r.part;
    SmoothArgs<TC, TS> a{};
    a.n = e->cap;
    a.mu_hist = static_cast<const TS*>(r.mu_hist_dev);
    a.cov_hist = static_cast<const TS*>(r.cov_hist_dev);
    a.mu_out = static_cast<TS*>(r.mu_out_dev);
    a.cov_out = static_cast<TS*>(r.cov_out_dev);
    const int64_t top = int64_t(p.top_slot) * e->cap;
    // the first launch starts from the filtered record of the window's last step, every other from what its predecessor stored
    a.start_mu = (p.first ? a.mu_hist : static_cast<const TS*>(a.mu_out)) + top * S;
    a.start_cov = p.first ? a.cov_hist + top * PK : static_cast<const TS*>(r.start_cov_dev);
    a.end_cov = static_cast<TS*>(r.end_cov_dev);
    a.copy_top = p.first ? ((r.mu_out_dev != r.mu_hist_dev ? 1 : 0) | ((r.cov_out_dev && r.cov_out_dev != r.cov_hist_dev) ? 2 : 0)) : 0;
    a.slots = r.slots;
    a.top_slot = p.top_slot;
    a.back = p.back;
    for (int k = 0; k < p.back && k < SMOOTH_MAX_BACK; ++k) a.dt[k] = r.dt[p.dt_first - k];
    a.initialised = e->init;
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
    a.status_accumulate = p.first ? 0 : 1;
    hipLaunchKernelGGL((ukf_smooth_kernel<TC, MC, TS>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("smoother kernel launch");
}

template <class M64, class M32> static int launch_smooth_model(ukfb_engine* e, const SmoothReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_smooth_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

}  // namespace ukfb
