// ukf_robust.hpp -- the robust sensor-frame update: ukf_sensor_meas_kernel's update with the noise covariance of an outlying
// sample inflated by a scalar, S(lambda) = Sigma_z + lambda Q, lambda >= 1.  Definitions: include/ukf_batch_robust.h,
// DESIGN.md 4.28.
//
// Layout, LDS map (sensor_map), models and every step but the scale are the sensor kernel's: its body
// (ukf_sensor_meas_body.inc.hpp) is included here with ROBUST true.  What this header adds is robust_scale, between the
// statistics (step 4) and the factorisation (step 6):
//  * it works on row-uniform scalars every lane of the row holds -- six entries of Sigma_z, six of Q, nu, lambda, f, g -- so it
//    needs no LDS and no row reduction, and four wave-mates with four models, m and trip counts take one code path;
//  * an evaluation at lambda is the 3 x 3 factorisation of S(lambda) by the pivot expressions of the sensor kernel's step 6,
//    y = Ls^-1 nu, x = Ls^-T y and the quadratic form g = x^T Q x; f = |y|^2 = d^2(lambda);
//  * MATCH: Newton on psi(lambda) = 1 / d^2(lambda) - 1 / c^2 from lambda = 1, lambda <- lambda + f (f - c^2) / (c^2 g).  psi is
//    concave and increasing, so the iterates rise towards the root and never pass it.  The loop has the shape of the mean
//    iteration: while (wave_any(active)) under a wave-uniform trip cap; a finished row rides along under selects;
//  * HUBER: lambda = sqrt(d0^2 / c^2), no loop.
// The entries beyond m (the identity in Sigma_z, zero in Q and nu) make m = 1 the same arithmetic: x = (y0 rs0, 0, 0).
#pragma once

#include "ukf_sensor_meas.hpp"

namespace ukfb {

// SensorArgs, the rule and the outputs the rule adds
template <class T, class TS> struct RobustArgs : SensorArgs<T, TS> {
    int mode;              // UKFB_ROBUST_MATCH / UKFB_ROBUST_HUBER
    T chi2_m1, chi2_m3;    // c^2 by the model's m
    T scale_max, tol;
    int max_iter;
    TS* maha0;             // [n] or null
    TS* scale;             // [n] or null
    int32_t* iterations;   // [n] or null
};
template <class T, class TS> inline constexpr bool sensor_args_robust<RobustArgs<T, TS>> = true;

// One evaluation at lambda: ok = the three pivots of S(lambda) are positive, f = nu^T S^-1 nu, g = x^T Q x with x = S^-1 nu
// (-g is the derivative of f in lambda)
template <class T> struct RobustEval {
    T f, g;
    bool ok;
};
template <class T> UKFB_DEV RobustEval<T> robust_eval(const T (&sz6)[6], const T (&q6)[6], const T (&nu)[3], T lam) {
    T s6[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) s6[i] = fma(lam, q6[i], sz6[i]);
    // (step 6 of the sensor kernel, pivot for pivot)
    const T d0 = s6[0], i0 = fast_rcp(d0);
    const T t10 = s6[1] * i0, t20 = s6[3] * i0;
    const T d1 = fma(-t10, s6[1], s6[2]), a21 = fma(-t20, s6[1], s6[4]);
    const T i1 = fast_rcp(d1);
    const T d2p = fma(-(a21 * i1), a21, fma(-t20, s6[3], s6[5]));
    RobustEval<T> e;
    e.ok = (d0 > T(0)) && (d1 > T(0)) && (d2p > T(0));   // (NaN fails every comparison)
    const T rs[3] = {fast_rsqrt(d0), fast_rsqrt(d1), fast_rsqrt(d2p)};
    const T l10 = s6[1] * rs[0], l20 = s6[3] * rs[0], l21 = a21 * rs[1];
    T y[3] = {nu[0], nu[1], nu[2]};
    sensor_solve3(y, l10, l20, l21, rs);
    e.f = fma(y[0], y[0], fma(y[1], y[1], y[2] * y[2]));
    // x = Ls^-T y
    const T x2 = y[2] * rs[2];
    const T x1 = fma(-l21, x2, y[1]) * rs[1];
    const T x0 = fma(-l20, x2, fma(-l10, x1, y[0])) * rs[0];
    const T qx0 = fma(q6[3], x2, fma(q6[1], x1, q6[0] * x0));
    const T qx1 = fma(q6[4], x2, fma(q6[2], x1, q6[1] * x0));
    const T qx2 = fma(q6[5], x2, fma(q6[4], x1, q6[3] * x0));
    e.g = fma(x2, qx2, fma(x1, qx1, x0 * qx0));
    return e;
}

// eligible: the row updates (live, a valid model, finite inputs, Sigma factorised).  Any other row, a row whose S(1) fails, a
// gated row and an inlier get lambda = 1 and no step: the body's step 6 then factorises Sigma_z + Q itself and judges it.
template <class T, class A>
UKFB_DEV RobustScale<T> robust_scale(const A& a, const T (&sz6)[6], const T (&q6)[6], const T (&nu)[3], int m, bool eligible) {
    RobustScale<T> r;
    const T c2 = (m == 1) ? a.chi2_m1 : a.chi2_m3;
    RobustEval<T> e = robust_eval(sz6, q6, nu, T(1));
    r.d0sq = e.f;
    r.accept = (a.gate_chi2 < T(0)) || (e.f <= a.gate_chi2);
    const bool inflate = eligible && e.ok && r.accept && (e.f > c2);
    T lam = T(1), f = e.f, g = e.g;
    int its = 0;
    if (a.mode == UKFB_ROBUST_HUBER) {   // (wave-uniform)
        lam = inflate ? m_sqrt(e.f / c2) : T(1);
    } else {
        bool active = inflate && (f - c2 > a.tol * c2);
        int trip = 0;
        while (wave_any(active) && trip < a.max_iter) {
            const T lam_new = lam + f * (f - c2) / (c2 * g);
            const bool go = active && (g > T(0)) && m_finite(g) && (lam_new > lam);
            lam = go ? lam_new : lam;
            its += go ? 1 : 0;
            e = robust_eval(sz6, q6, nu, lam);
            f = go ? e.f : f;
            g = go ? e.g : g;
            active = go && e.ok && (f - c2 > a.tol * c2) && (lam < a.scale_max) && (its < a.max_iter);
            ++trip;
        }
    }
    r.lam = m_min(lam, a.scale_max);
    r.its = its;
    return r;
}

template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_robust_kernel(const RobustArgs<T, TS> a) {
#include "ukf_sensor_meas_body.inc.hpp"
}

}  // namespace ukfb
