// ukf_feature_launch.hpp -- what the typed launches of the feature kernels (ukf_*_launch.inc.hpp) share: the choice of the
// three instantiations of a model by the engine's precision.
#pragma once

#include "ukf_engine.hpp"

namespace ukfb {

// storage type, model at the compute type's precision class, compute type: the template arguments of a launch_*_typed
template <class TS_, class M_, class TC_> struct Precision {
    using TS = TS_;
    using M = M_;
    using TC = TC_;
};

// f(Precision<...>{}) for the engine's mode: fp64, fp32 arrays with fp64 arithmetic (wide_arithmetic), fp32
template <class M64, class M32, class F> static int dispatch_precision(const ukfb_engine* e, F&& f) {
    if (e->prec == UKFB_F64) return f(Precision<double, M64, double>{});
    if (e->cfg.wide_arithmetic) return f(Precision<float, M32, double>{});
    return f(Precision<float, M32, float>{});
}

}  // namespace ukfb
