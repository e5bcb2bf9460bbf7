// ukf_condition_launch.inc.hpp -- typed launches of ukf_condition_kernel<T, M, TS>; included by the two per-model translation
// units.  The three instantiations of a model: fp64, fp32, fp32 arrays with fp64 arithmetic (wide_arithmetic).
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_condition.hpp"
#include "ukf_condition_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_condition_typed(ukfb_engine* e, const ConditionReq& r) {
    using MC = typename M::template rebind<TC>;
    const RowGeometry geo = condition_geometry(MC::S, MC::D, e->cap, sizeof(TC));
    if (geo.grid == 0) return UKFB_OK;
    ConditionArgs<TC, TS> a{};
    a.n = e->cap;
    a.mu = static_cast<const TS*>(e->mu);
    a.cov = static_cast<const TS*>(e->cov);
    // commit = 0: the kernel gets no pointer through which it could store to the engine
    a.mu_out = r.commit ? static_cast<TS*>(e->mu) : nullptr;
    a.cov_out = r.commit ? static_cast<TS*>(e->cov) : nullptr;
    a.engine_status = r.commit ? e->status : nullptr;
    a.initialised = e->init;
    a.var_floor = static_cast<const TS*>(r.in.var_floor_dev);
    a.eig_floor = TC(r.in.eig_floor);
    a.select = r.in.select_dev;
    a.renormalize = r.in.renormalize_quaternion;
    a.eig_min = static_cast<TS*>(r.out.eig_min);
    a.eig_max = static_cast<TS*>(r.out.eig_max);
    a.mu_o = static_cast<TS*>(r.out.mu);
    a.cov_packed = static_cast<TS*>(r.out.cov_packed);
    a.status = r.out.status;
    hipLaunchKernelGGL((ukf_condition_kernel<TC, MC, TS>), dim3((unsigned)geo.grid), dim3(64), size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("conditioning kernel launch");
}

template <class M64, class M32> static int launch_condition_model(ukfb_engine* e, const ConditionReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_condition_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

}  // namespace ukfb
