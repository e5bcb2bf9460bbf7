// ukf_delayed_launch.hpp -- the arguments that ukf_delayed_kernel and ukf_relative_kernel<T, M, TS> share: both take
// DelayedArgs over the history window of a request whose `in` and `out` differ only in the names of the model fields.
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_delayed.hpp"

namespace ukfb {

template <class TS, class MC, class TC, class Req>
DelayedArgs<TC, TS> delayed_args(const ukfb_engine* e, const Req& r, int model_uniform, const int32_t* model_dev) {
    DelayedArgs<TC, TS> a{};
    bind_state<TS>(a, e, r.commit, a.eng_mu, a.eng_cov);   // (mu_out / cov_out are the caller's)
    a.mu_hist = static_cast<const TS*>(r.in.mu_hist_dev);
    a.cov_hist = static_cast<const TS*>(r.in.cov_hist_dev);
    a.slots = r.in.slots;
    a.back = r.in.steps - 1;
    a.top_slot = int((int64_t(r.in.first_slot) + a.back) % r.in.slots);
    for (int k = 0; k < a.back && k < SMOOTH_MAX_BACK; ++k) a.dt[k] = r.in.dt[a.back - 1 - k];
    bind_process<TS, TC>(a, e, MC::D, r.in.in_a_dev, r.in.in_b_dev);
    a.lag_uniform = r.in.lag_uniform;
    a.lag = r.in.lag_dev;
    a.model_uniform = model_uniform;
    a.model = model_dev;
    a.z = static_cast<const TS*>(r.in.z_dev);
    a.Q = static_cast<const TS*>(r.in.Q_dev);
    a.q_uniform = r.in.q_is_uniform;
    bind_gate<TS, TC>(a, e);
    a.z_pred = static_cast<TS*>(r.out.z_pred);
    a.S = static_cast<TS*>(r.out.S);
    a.innov = static_cast<TS*>(r.out.innov);
    a.maha = static_cast<TS*>(r.out.maha);
    a.loglik = static_cast<TS*>(r.out.loglik);
    a.status = r.out.status;
    a.mu_out = static_cast<TS*>(r.out.mu_out);
    a.cov_out = static_cast<TS*>(r.out.cov_out);
    return a;
}

}  // namespace ukfb
