// ukf_condition_launch.hip -- typed launch of ukf_condition_kernel<T, M, TS>
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_condition.hpp"

namespace ukfb {

template <> struct FeatureLaunch<ConditionReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const ConditionReq& r) {
        const RowGeometry geo = condition_geometry(MC::S, MC::D, e->cap, sizeof(TC));
        ConditionArgs<TC, TS> a{};
        bind_state<TS>(a, e, r.commit);
        a.var_floor = static_cast<const TS*>(r.in.var_floor_dev);
        a.eig_floor = TC(r.in.eig_floor);
        a.select = r.in.select_dev;
        a.renormalize = r.in.renormalize_quaternion;
        a.eig_min = static_cast<TS*>(r.out.eig_min);
        a.eig_max = static_cast<TS*>(r.out.eig_max);
        a.mu_o = static_cast<TS*>(r.out.mu);
        a.cov_packed = static_cast<TS*>(r.out.cov_packed);
        a.status = r.out.status;
        return launch_rows(e, ukf_condition_kernel<TC, MC, TS>, geo, "conditioning kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(ConditionReq)

}  // namespace ukfb
