// ukf_smooth_launch.hip -- typed launch of ukf_smooth_kernel<T, M, TS>
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_smooth.hpp"

namespace ukfb {

template <> struct FeatureLaunch<SmoothReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const SmoothReq& r) {
        constexpr int S = MC::S, D = MC::D, PK = D * (D + 1) / 2;
        const RowGeometry geo = smooth_geometry(S, D, e->cap, sizeof(TC));
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
        bind_process<TS, TC>(a, e, D, r.in_a_dev, r.in_b_dev);
        a.status = r.status_dev;
        a.status_accumulate = p.first ? 0 : 1;
        return launch_rows(e, ukf_smooth_kernel<TC, MC, TS>, geo, "smoother kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(SmoothReq)

}  // namespace ukfb
