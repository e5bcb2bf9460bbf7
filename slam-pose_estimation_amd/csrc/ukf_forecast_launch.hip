// ukf_forecast_launch.hip -- typed launch of ukf_forecast_kernel<T, M, TS>
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_forecast.hpp"

namespace ukfb {

template <> struct FeatureLaunch<ForecastReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const ForecastReq& r) {
        const RowGeometry geo = forecast_geometry(MC::S, MC::D, e->cap, sizeof(TC));
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
        bind_process<TS, TC>(a, e, MC::D, r.in_a_dev, r.in_b_dev);
        a.status = r.status_dev;
        return launch_rows(e, ukf_forecast_kernel<TC, MC, TS>, geo, "forecast kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(ForecastReq)

}  // namespace ukfb
