// ukf_bank_launch.inc.hpp -- typed launches of the filter-bank kernels; included by the two per-model translation units.
// The three instantiations of a model: fp64, fp32, fp32 arrays with fp64 arithmetic (wide_arithmetic).
#pragma once

#include <limits>

#include "ukf_feature_launch.hpp"
#include "ukf_bank.hpp"
#include "ukf_bank_req.hpp"

namespace ukfb {

template <class TS, class M, class TC> static int launch_bank_typed(ukfb_engine* e, const BankReq& r) {
    using MC = typename M::template rebind<TC>;
    const BankGeometry geo = bank_geometry(MC::S, MC::D, r.hypotheses, e->cap, sizeof(TC));
    if (geo.grid == 0) return UKFB_OK;
    BankArgs<TC, TS> a{};
    a.tracks = geo.tracks;
    a.hyp = r.hypotheses;
    a.mu_in = static_cast<const TS*>(e->mu);
    a.cov_in = static_cast<const TS*>(e->cov);
    a.initialised = e->init;
    a.w = static_cast<const TS*>(r.w_dev);
    a.mean_tol = TC(e->cfg.mean_tol);
    a.mean_max_it = e->cfg.mean_max_iter;
    a.sum_tol = TC(16.0 * r.hypotheses * double(std::numeric_limits<TS>::epsilon()));
    a.status = r.status_dev;
    const dim3 grid((unsigned)geo.grid), block(64);
    if (r.mix) {
        a.mu_out = static_cast<TS*>(e->mu);
        a.cov_out = static_cast<TS*>(e->cov);
        a.w_pred = static_cast<TS*>(r.w_pred_dev);
        for (int k = 0; k < r.hypotheses * r.hypotheses; ++k) a.Pi[k] = TC(r.transition[k]);
        hipLaunchKernelGGL((ukf_bank_mix_kernel<TC, MC, TS>), grid, block, size_t(geo.lds_bytes), main_stream(e), a);
        return launch_status("bank mix kernel launch");
    }
    a.mu_out = static_cast<TS*>(r.mu_out_dev);
    a.cov_out = static_cast<TS*>(r.cov_out_dev);
    hipLaunchKernelGGL((ukf_bank_combine_kernel<TC, MC, TS>), grid, block, size_t(geo.lds_bytes), main_stream(e), a);
    return launch_status("bank combine kernel launch");
}

template <class M64, class M32> static int launch_bank_model(ukfb_engine* e, const BankReq& r) {
    return dispatch_precision<M64, M32>(e, [&](auto p) {
        using P = decltype(p);
        return launch_bank_typed<typename P::TS, typename P::M, typename P::TC>(e, r);
    });
}

template <class TS, class TC> static int launch_bank_weights_typed(ukfb_engine* e, const BankWeightsReq& r) {
    BankWeightArgs<TC, TS> a{};
    a.tracks = e->cap / r.hypotheses;
    a.hyp = r.hypotheses;
    a.logw_in = static_cast<const TS*>(r.logw_in_dev);
    a.loglik = static_cast<const TS*>(r.loglik_dev);
    a.logw_out = static_cast<TS*>(r.logw_out_dev);
    a.w_out = static_cast<TS*>(r.w_out_dev);
    a.status = r.status_dev;
    if (a.tracks == 0) return UKFB_OK;
    hipLaunchKernelGGL((ukf_bank_weights_kernel<TC, TS>), dim3((unsigned)((a.tracks + 255) / 256)), dim3(256), 0, main_stream(e), a);
    return launch_status("bank weights kernel launch");
}

}  // namespace ukfb
