// ukf_innovation_launch.hip -- typed launch of ukf_innovation_kernel<T, M, TS>
#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_innovation.hpp"

namespace ukfb {

template <> struct FeatureLaunch<InnovReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const InnovReq& r) {
        InnovArgs<TS> a{};
        a.n = e->cap;
        a.mu = static_cast<const TS*>(e->mu);
        a.cov = static_cast<const TS*>(e->cov);
        a.initialised = e->init;
        a.meas_uniform = r.meas_uniform;
        a.meas = r.meas_dev;
        a.candidates = r.candidates;
        a.z = static_cast<const TS*>(r.z_dev);
        a.Q = static_cast<const TS*>(r.Q_dev);
        a.q_uniform = r.q_uniform ? 1 : 0;
        a.mean_tol = TS(e->cfg.mean_tol);   // (this kernel takes its scalars in the storage type)
        a.mean_max_it = e->cfg.mean_max_iter;
        a.gate_chi2 = TS(e->cfg.gate_chi2);
        a.z_pred = static_cast<TS*>(r.out.z_pred);
        a.S = static_cast<TS*>(r.out.S);
        a.innov = static_cast<TS*>(r.out.innov);
        a.maha = static_cast<TS*>(r.out.maha);
        a.loglik = static_cast<TS*>(r.out.loglik);
        a.best = r.out.best;
        a.status = r.out.status;
        const RowGeometry geo{(a.n + 3) / 4, 0};   // four filters per workgroup, no LDS
        return launch_rows(e, ukf_innovation_kernel<TC, MC, TS>, geo, "innovation kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(InnovReq)

}  // namespace ukfb
