// ukf_bank_launch.hip -- typed launches of the filter-bank kernels: ukf_bank_mix_kernel / ukf_bank_combine_kernel<T, M, TS>
// and, in the Pose object, the model-independent ukf_bank_weights_kernel<T, TS>
#include <limits>

#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_bank.hpp"

namespace ukfb {

template <> struct FeatureLaunch<BankReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const BankReq& r) {
        const BankGeometry geo = bank_geometry(MC::S, MC::D, r.hypotheses, e->cap, sizeof(TC));
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
        if (r.mix) {
            a.mu_out = static_cast<TS*>(e->mu);
            a.cov_out = static_cast<TS*>(e->cov);
            a.w_pred = static_cast<TS*>(r.w_pred_dev);
            for (int k = 0; k < r.hypotheses * r.hypotheses; ++k) a.Pi[k] = TC(r.transition[k]);
            return launch_rows(e, ukf_bank_mix_kernel<TC, MC, TS>, geo, "bank mix kernel launch", a);
        }
        a.mu_out = static_cast<TS*>(r.mu_out_dev);
        a.cov_out = static_cast<TS*>(r.cov_out_dev);
        return launch_rows(e, ukf_bank_combine_kernel<TC, MC, TS>, geo, "bank combine kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(BankReq)

#ifdef UKFB_LAUNCH_POSE
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
    // (a track per lane, not launch_rows' wavefront per workgroup)
    hipLaunchKernelGGL((ukf_bank_weights_kernel<TC, TS>), dim3((unsigned)((a.tracks + 255) / 256)), dim3(256), 0, main_stream(e), a);
    return launch_status("bank weights kernel launch");
}

int launch_bank_weights(ukfb_engine* e, const BankWeightsReq& r) {
    return dispatch_precision<void, void>(e, [&](auto p) {   // (no model)
        using P = decltype(p);
        return launch_bank_weights_typed<typename P::TS, typename P::TC>(e, r);
    });
}
#endif

}  // namespace ukfb
