// ukf_predict_sampled_launch.hip -- typed launch of ukf_predict_sampled_kernel<T, M, TS>
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_predict_sampled.hpp"

namespace ukfb {

template <> struct FeatureLaunch<PredictSampledReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const PredictSampledReq& r) {
        const RowGeometry geo = predict_sampled_geometry(MC::S, MC::D, e->cap, sizeof(TC));
        PredictSampledArgs<TC, TS> a{};
        a.n = e->cap;
        bind_commit<TS>(a, e, r.commit);   // (the kernel reads the propagated points, not the engine's state: a.mu is an output)
        a.initialised = e->init;
        a.XX = static_cast<const TS*>(r.in.XX_dev);
        a.R = static_cast<const TS*>(r.in.R_dev);
        a.R_stride = r.in.r_is_uniform ? 0 : int64_t(MC::D) * MC::D;
        a.active = r.in.active_dev;
        bind_mean<TS, TC>(a, e);
        a.mu = static_cast<TS*>(r.out.mu);
        a.cov_packed = static_cast<TS*>(r.out.cov_packed);
        a.status = r.out.status;
        return launch_rows(e, ukf_predict_sampled_kernel<TC, MC, TS>, geo, "sampled-prediction kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(PredictSampledReq)

}  // namespace ukfb
