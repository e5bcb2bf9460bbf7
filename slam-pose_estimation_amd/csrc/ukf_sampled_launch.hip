// ukf_sampled_launch.hip -- typed launches of ukf_sigma_points_kernel and ukf_sampled_kernel<T, M, TS>
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_sampled.hpp"

namespace ukfb {

template <> struct FeatureLaunch<SigmaPointsReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const SigmaPointsReq& r) {
        const RowGeometry geo = sigma_points_geometry(MC::S, MC::D, e->cap, sizeof(TC));
        SigmaPointsArgs<TC, TS> a{};
        a.n = e->cap;
        a.mu = static_cast<const TS*>(e->mu);
        a.cov = static_cast<const TS*>(e->cov);
        a.initialised = e->init;
        a.X = static_cast<TS*>(r.X);
        a.delta = static_cast<TS*>(r.delta);
        a.status = r.status;
        return launch_rows(e, ukf_sigma_points_kernel<TC, MC, TS>, geo, "sigma-point export kernel launch", a);
    }
};

template <> struct FeatureLaunch<SampledReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const SampledReq& r) {
        const RowGeometry geo = sampled_geometry(MC::S, MC::D, e->cap, sizeof(TC));
        SampledArgs<TC, TS> a{};
        bind_state<TS>(a, e, r.commit);
        a.m = r.in.m;
        a.Z = static_cast<const TS*>(r.in.Z_dev);
        a.z = static_cast<const TS*>(r.in.z_dev);
        a.Q = static_cast<const TS*>(r.in.Q_dev);
        a.q_uniform = r.in.q_is_uniform;
        a.active = r.in.active_dev;
        bind_mean<TS, TC>(a, e);
        bind_gate<TS, TC>(a, e);
        a.z_pred = static_cast<TS*>(r.out.z_pred);
        a.S = static_cast<TS*>(r.out.S);
        a.innov = static_cast<TS*>(r.out.innov);
        a.maha = static_cast<TS*>(r.out.maha);
        a.loglik = static_cast<TS*>(r.out.loglik);
        a.status = r.out.status;
        return launch_rows(e, ukf_sampled_kernel<TC, MC, TS>, geo, "sampled-update kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(SigmaPointsReq)
UKFB_LAUNCH_UNIT(SampledReq)

}  // namespace ukfb
