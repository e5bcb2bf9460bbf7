// ukf_state_meas_launch.hip -- typed launch of ukf_state_meas_kernel<T, M, TS>
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_state_meas.hpp"

namespace ukfb {

template <> struct FeatureLaunch<StateMeasReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const StateMeasReq& r) {
        const RowGeometry geo = state_meas_geometry(MC::S, MC::D, e->cap, sizeof(TC));
        StateMeasArgs<TC, TS> a{};
        bind_state<TS>(a, e, r.commit);
        a.mask_uniform = r.mask_uniform;
        a.mask = r.mask_dev;
        a.z = static_cast<const TS*>(r.z_dev);
        a.Qz = static_cast<const TS*>(r.Qz_dev);
        a.infl_state = TC(r.state_inflation);
        a.infl_meas = TC(r.meas_inflation);
        bind_mean<TS, TC>(a, e);
        bind_gate<TS, TC>(a, e);
        a.maha = static_cast<TS*>(r.out.maha);
        a.loglik = static_cast<TS*>(r.out.loglik);
        a.status = r.out.status;
        return launch_rows(e, ukf_state_meas_kernel<TC, MC, TS>, geo, "state-measurement kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(StateMeasReq)

}  // namespace ukfb
