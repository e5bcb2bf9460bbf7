// ukf_relative_launch.hip -- typed launch of ukf_relative_kernel<T, M, TS>; the feature has PoseWithVelocity kernels only
#include "ukf_delayed_launch.hpp"
#include "ukf_relative.hpp"

namespace ukfb {

template <> struct FeatureLaunch<RelativeReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const RelativeReq& r) {
        const RowGeometry geo = relative_geometry(MC::S, MC::D, e->cap, sizeof(TC));
        const RelativeArgs<TC, TS> a = delayed_args<TS, MC, TC>(e, r, r.in.model_uniform, r.in.model_dev);
        return launch_rows(e, ukf_relative_kernel<TC, MC, TS>, geo, "relative-measurement kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(RelativeReq)

}  // namespace ukfb
