// ukf_pda_launch.hip -- typed launch of ukf_pda_kernel<T, M, TS>: the shared-h association launch with the rule's three
// logarithms and the outputs the weights add
#include <cmath>

#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_pda.hpp"

namespace ukfb {

template <> struct FeatureLaunch<PdaReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const PdaReq& r) {
        const RowGeometry geo = sensor_geometry(MC::S, MC::D, e->cap, sizeof(TC));   // the sensor kernel's LDS map
        PdaArgs<TC, TS> a{};
        bind_state<TS>(a, e, r.commit);
        bind_sensor_inputs<TS, TC>(a, e, r, /*gyro*/ true);
        a.candidates = r.in.candidates;
        bind_mean<TS, TC>(a, e);
        bind_gate<TS, TC>(a, e);
        const PdaLogs lg = pda_logs(r.rule);   // formed in double
        a.a0_m1 = TC(TS(lg.a0_m1));
        a.a0_m3 = TC(TS(lg.a0_m3));
        a.ln_pd = TC(TS(lg.ln_pd));
        a.beta = static_cast<TS*>(r.out.beta);
        a.beta0 = static_cast<TS*>(r.out.beta0);
        a.innov_comb = static_cast<TS*>(r.out.innov_comb);
        a.best = r.out.best;
        a.n_gated = r.out.n_gated;
        return launch_rows(e, ukf_pda_kernel<TC, MC, TS>, geo, "probabilistic-association kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(PdaReq)

}  // namespace ukfb
