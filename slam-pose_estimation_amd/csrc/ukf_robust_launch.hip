// ukf_robust_launch.hip -- ukf_robust_kernel<T, M, TS> behind the robust sensor-frame update: the sensor-frame launch with the
// rule and the outputs the rule adds
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_robust.hpp"

namespace ukfb {

template <> struct FeatureLaunch<RobustReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const RobustReq& r) {
        const RowGeometry geo = sensor_geometry(MC::S, MC::D, e->cap, sizeof(TC));   // the sensor kernel's LDS map
        RobustArgs<TC, TS> a{};
        bind_state<TS>(a, e, r.commit);
        bind_sensor_inputs<TS, TC>(a, e, r, /*gyro*/ true);
        bind_mean<TS, TC>(a, e);
        bind_gate<TS, TC>(a, e);
        a.mode = r.rule.mode;
        a.chi2_m1 = TC(TS(r.rule.chi2_m1));
        a.chi2_m3 = TC(TS(r.rule.chi2_m3));
        a.scale_max = TC(TS(r.rule.scale_max));
        a.tol = TC(TS(r.rule.tol));
        a.max_iter = r.rule.max_iter;
        a.maha0 = static_cast<TS*>(r.out.maha0);
        a.scale = static_cast<TS*>(r.out.scale);
        a.iterations = r.out.iterations;
        return launch_rows(e, ukf_robust_kernel<TC, MC, TS>, geo, "robust sensor-measurement kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(RobustReq)

}  // namespace ukfb
