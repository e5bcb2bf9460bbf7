// ukf_associate_launch.hip -- typed launch of ukf_associate_kernel<T, M, TS, HYP>, in the shared-h and the per-hypothesis mode
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_associate.hpp"

namespace ukfb {

template <> struct FeatureLaunch<AssociateReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const AssociateReq& r) {
        const RowGeometry geo = sensor_geometry(MC::S, MC::D, e->cap, sizeof(TC));   // the sensor kernel's LDS map
        AssociateArgs<TC, TS> a{};
        bind_state<TS>(a, e, r.commit);
        bind_sensor_inputs<TS, TC>(a, e, r, true);
        a.candidates = r.in.candidates;
        bind_mean<TS, TC>(a, e);
        bind_gate<TS, TC>(a, e);
        a.best = r.out.best;
        a.n_gated = r.out.n_gated;
        return launch_rows(e, r.in.point_per_candidate ? ukf_associate_kernel<TC, MC, TS, true> : ukf_associate_kernel<TC, MC, TS, false>,
                           geo, "sensor-association kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(AssociateReq)

}  // namespace ukfb
