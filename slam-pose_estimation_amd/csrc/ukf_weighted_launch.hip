// ukf_weighted_launch.hip -- typed launch of ukf_weighted_kernel<T, M, TS>: the shared-h association launch without a gate,
// with the weights to read and the outputs they add
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_weighted.hpp"

namespace ukfb {

template <> struct FeatureLaunch<WeightedReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const WeightedReq& r) {
        const RowGeometry geo = sensor_geometry(MC::S, MC::D, e->cap, sizeof(TC));   // the sensor kernel's LDS map
        WeightedArgs<TC, TS> a{};
        bind_state<TS>(a, e, r.commit);
        bind_sensor_inputs<TS, TC>(a, e, r, /*gyro*/ true);
        a.candidates = r.in.candidates;
        bind_mean<TS, TC>(a, e);
        a.weight = static_cast<const TS*>(r.weight);
        a.weight_used = static_cast<TS*>(r.out.weight_used);
        a.beta0 = static_cast<TS*>(r.out.beta0);
        a.innov_comb = static_cast<TS*>(r.out.innov_comb);
        a.n_used = r.out.n_used;
        return launch_rows(e, ukf_weighted_kernel<TC, MC, TS>, geo, "weighted-update kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(WeightedReq)

}  // namespace ukfb
