// ukf_predict_sampled_launch.inc.hpp -- typed launches of ukf_predict_sampled_kernel<T, M, TS>; included by the two per-model
// translation units.  The three instantiations of a model: fp64, fp32, fp32 arrays with fp64 arithmetic (wide_arithmetic).
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_predict_sampled.hpp"
#include "ukf_predict_sampled_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_predict_sampled_typed(ukfb_engine* e, const PredictSampledReq& r) {
    using MC = typename M::template rebind<TC>;
    const RowGeometry geo = predict_sampled_geometry(MC::S, MC::D, e->cap, sizeof(TC));
    if (geo.grid == 0) return UKFB_OK;
    PredictSampledArgs<TC, TS> a{};
    a.n = e->cap;
    // commit = 0: the kernel gets no pointer through which it could store to the engine
    a.mu_out = r.commit ? static_cast<TS*>(e->mu) : nullptr;
    a.cov_out = r.commit ? static_cast<TS*>(e->cov) : nullptr;
    a.engine_status = r.commit ? e->status : nullptr;
    a.initialised = e->init;
    a.XX = static_cast<const TS*>(r.in.XX_dev);
    a.R = static_cast<const TS*>(r.in.R_dev);
    a.R_stride = r.in.r_is_uniform ? 0 : int64_t(MC::D) * MC::D;
    a.active = r.in.active_dev;
    a.mean_tol = TC(TS(e->cfg.mean_tol));   // (rounded as the forward launches round them)
    a.mean_max_it = e->cfg.mean_max_iter;
    a.mu = static_cast<TS*>(r.out.mu);
    a.cov_packed = static_cast<TS*>(r.out.cov_packed);
    a.status = r.out.status;
    hipLaunchKernelGGL((ukf_predict_sampled_kernel<TC, MC, TS>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("sampled-prediction kernel launch");
}

template <class M64, class M32> static int launch_predict_sampled_model(ukfb_engine* e, const PredictSampledReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_predict_sampled_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

}  // namespace ukfb
