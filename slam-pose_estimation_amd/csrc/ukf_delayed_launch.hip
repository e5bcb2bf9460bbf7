// ukf_delayed_launch.hip -- typed launch of ukf_delayed_kernel<T, M, TS>
#include "ukf_delayed_launch.hpp"

namespace ukfb {

template <> struct FeatureLaunch<DelayedReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const DelayedReq& r) {
        const RowGeometry geo = delayed_geometry(MC::S, MC::D, e->cap, sizeof(TC));
        const DelayedArgs<TC, TS> a = delayed_args<TS, MC, TC>(e, r, r.in.meas_model_uniform, r.in.meas_model_dev);
        return launch_rows(e, ukf_delayed_kernel<TC, MC, TS>, geo, "delayed-measurement kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(DelayedReq)

}  // namespace ukfb
