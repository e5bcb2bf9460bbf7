// ukf_sensor_meas.hpp -- sensor-frame measurements: ukfom's update with a nonlinear h that knows where the sensor is mounted
// (lever arm r, sensor -> body rotation qs) and / or a nav-frame point b, measurement space R^m with m = 1 or 3, per-filter
// model ids, a read-only mode.  Definitions: include/ukf_batch.h ("sensor-frame measurements"), DESIGN.md 4.17.
//
// Layout: the state-measurement kernel's (ukf_state_meas.hpp) -- one filter per 16-lane DPP row, four per wavefront, one
// wavefront per workgroup -- and its device functions: chol16 / load_column / sigma_pair, row_boxplus, the applyDelta commit.
//  * lane l < D owns the sigma pair of factor column l and evaluates h on both points; lane D owns the centre.
//  * the measurement side is three-dimensional whatever the model: m = 1 is embedded with zero deltas, identity rows / columns
//    of S and nu = 0 there (the argument of ukf_state_meas.hpp for unselected dimensions), so that four wave-mates with four
//    model ids take one code path.  The models of an engine differ by per-row selects of the operands of three rotations; a
//    rotation no row of the wavefront needs is skipped by a wave-uniform branch whose result no other row reads.
//  * S is six row all-reductions of u u^T + w w^T (u, w = half sum / half difference of the lane's two deltas; the centre adds
//    delta_0 delta_0^T / 2); S, its factor and y = Ls^-1 nu live in registers on every lane of the row.
//  * C row l = sum_j L[l][j] W_j^T: the factor columns and the D x 3 half differences from LDS with row-uniform reads; the row is
//    solved against Ls in registers (Y = C Ls^-T), and only the D x 3 matrix Y goes through LDS for Sigma~ = Sigma - Y Y^T.
//  * the per-filter inputs (z, Q, mount, point: 22 scalars) are staged once: lane i takes entries i and i + 16, judges its own
//    (used by the row's model and not finite: ERR_NONFINITE_MEAS) and stores the entry or, if the model does not read it, its
//    neutral value -- a NaN in an unused entry never meets arithmetic.
//  * differences are formed before rotating (p - b, then + R(q) r; R(q)^T (b - p)), so that fp32 does not subtract two large
//    rotated vectors; h and the differences Z_i - Z_0, z - Z_0 are evaluated in fp64 in every mode, and the mean iteration, the
//    deltas and the innovation work on those differences (the same iteration on a vector space, with an iterate small enough for
//    mean_tol to mean something in fp32).
//  * a filter that fails, is gated, inactive or uninitialised rides along: every select is per row, no row's bits depend on its
//    wave-mates (the mean iteration runs while any row is active; a converged row keeps its reference).
//  * commit = 0: the kernel gets NULL for the state's output pointers -- it has nothing through which it could store.
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
// LDS per filter: sensor_map (ukf_host.hpp).
#pragma once

#include "ukf_row.hpp"

namespace ukfb {

template <class T, class TS> struct SensorArgs {
    int64_t n;                   // filters
    const TS* mu;                // [n][S]
    const TS* cov;               // [n][PK]
    TS* mu_out;                  // the same arrays for commit = 1, null for commit = 0
    TS* cov_out;
    uint32_t* engine_status;     // [n]; null for commit = 0
    const uint8_t* initialised;  // [n]
    int model_uniform;
    const int32_t* model;        // [n] or null
    const TS* z;                 // [n][3]
    const TS* Q;                 // [n][9], or [9] when q_uniform
    int q_uniform;
    const TS* mount;             // [n][7] or null: mount_u
    const TS* point;             // [n][3] or null: point_u
    T mount_u[7], point_u[3];
    const TS* gyro;              // OrientationState: the latched rotation rate [n][3]
    T mean_tol;
    int mean_max_it;
    T gate_chi2;                 // < 0: accept
    TS* z_pred;                  // [n][3] or null
    TS* S;                       // [n][9] or null
    TS* innov;                   // [n][3] or null
    TS* maha;                    // [n] or null
    TS* loglik;                  // [n] or null
    uint32_t* status;            // [n] or null
};


// What h reads beside the sigma point: the (neutralised) mount and point, the inverse of qs, 1 / |q|^2 of the mean's
// orientation (every sigma point's orientation is the mean's times a unit exponential) and, OrientationState, the gyro sample
template <class T> struct SensorIn {
    T r[3], qsi[4], b[3], gy[3], rnq;
};

// PoseWithVelocity: ids 0 ... 4 (include/ukf_batch.h); need_* are wave-uniform
template <class T>
UKFB_DEV void sensor_h(PoseM<T>*, const T (&x)[13], int id, const SensorIn<T>& in, bool need_fwd, bool need_point, bool need_sens, T (&z)[3]) {
    const T q[4] = {x[3], x[4], x[5], x[6]};
    const T d[3] = {x[0] - in.b[0], x[1] - in.b[1], x[2] - in.b[2]};   // p - b before anything is rotated
    const bool nav = id == UKFB_SENSOR_POSE_NAV_VELOCITY, pnt = id == UKFB_SENSOR_POSE_POINT;
    const bool sens = pnt || id == UKFB_SENSOR_POSE_VELOCITY;
    T u[3] = {T(0), T(0), T(0)}, g[3] = {T(0), T(0), T(0)}, o[3] = {T(0), T(0), T(0)};
    if (need_fwd) {   // POSITION, RANGE: (p - b) + R(q) r; NAV_VELOCITY: R(q) v
        const T fin[3] = {nav ? x[7] : in.r[0], nav ? x[8] : in.r[1], nav ? x[9] : in.r[2]};
        T f[3];
        quat_rotate(q, fin, f);
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = nav ? f[c] : (d[c] + f[c]);
    }
    if (need_point) {   // POINT: R(q)^T (b - p) - r
        const T qi[4] = {-q[0] * in.rnq, -q[1] * in.rnq, -q[2] * in.rnq, q[3] * in.rnq};
        const T nb[3] = {-d[0], -d[1], -d[2]};
        quat_rotate(qi, nb, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] -= in.r[c];
    }
    if (need_sens) {   // POINT, VELOCITY: R(qs)^T (...); VELOCITY: v + omega x r
        const T w[3] = {x[10], x[11], x[12]};
        const T pre[3] = {pnt ? g[0] : x[7] + (w[1] * in.r[2] - w[2] * in.r[1]), pnt ? g[1] : x[8] + (w[2] * in.r[0] - w[0] * in.r[2]),
                          pnt ? g[2] : x[9] + (w[0] * in.r[1] - w[1] * in.r[0])};
        quat_rotate(in.qsi, pre, o);
    }
    const bool rng = id == UKFB_SENSOR_POSE_RANGE;
    const T nrm = m_sqrt(fma(u[0], u[0], fma(u[1], u[1], u[2] * u[2])));
    z[0] = sens ? o[0] : (rng ? nrm : u[0]);
    z[1] = sens ? o[1] : (rng ? T(0) : u[1]);
    z[2] = sens ? o[2] : (rng ? T(0) : u[2]);
}

// OrientationState: ids 5 ... 7
template <class T>
UKFB_DEV void sensor_h(OrientM<T>*, const T (&x)[14], int id, const SensorIn<T>& in, bool, bool, bool need_sens, T (&z)[3]) {
    const T q[4] = {x[0], x[1], x[2], x[3]};
    const T qi[4] = {-q[0] * in.rnq, -q[1] * in.rnq, -q[2] * in.rnq, q[3] * in.rnq};
    const bool vel = id == UKFB_SENSOR_ORIENT_VELOCITY, vec = id == UKFB_SENSOR_ORIENT_NAV_VECTOR;
    const T iin[3] = {vel ? x[4] : (vec ? in.b[0] : T(0)), vel ? x[5] : (vec ? in.b[1] : T(0)), vel ? x[6] : (vec ? in.b[2] : x[13])};
    T i3[3], o[3] = {T(0), T(0), T(0)};
    quat_rotate(qi, iin, i3);   // R(q)^T v, R(q)^T b, R(q)^T (0, 0, g)
    if (need_sens) {   // VELOCITY, NAV_VECTOR: R(qs)^T (...); VELOCITY: + (w_gyro - b_g) x r
        const T w[3] = {in.gy[0] - x[7], in.gy[1] - x[8], in.gy[2] - x[9]};
        const T pre[3] = {i3[0] + (vel ? (w[1] * in.r[2] - w[2] * in.r[1]) : T(0)), i3[1] + (vel ? (w[2] * in.r[0] - w[0] * in.r[2]) : T(0)),
                          i3[2] + (vel ? (w[0] * in.r[1] - w[1] * in.r[0]) : T(0))};
        quat_rotate(in.qsi, pre, o);
    }
    const bool sf = !(vel || vec);   // SPECIFIC_FORCE: + b_a
    z[0] = sf ? (i3[0] + x[10]) : o[0];
    z[1] = sf ? (i3[1] + x[11]) : o[1];
    z[2] = sf ? (i3[2] + x[12]) : o[2];
}

// c <- Ls^-1 c for the 3 x 3 factor held as (l10, l20, l21) and the reciprocal pivots' roots rs
template <class T> UKFB_DEV void sensor_solve3(T (&c)[3], T l10, T l20, T l21, const T (&rs)[3]) {
    c[0] = c[0] * rs[0];
    c[1] = fma(-l10, c[0], c[1]) * rs[1];
    c[2] = fma(-l21, c[1], fma(-l20, c[0], c[2])) * rs[2];
}

// ROBUST (ukf_robust.hpp): what the robust update finds between steps 5 and 6 -- the scale lambda of Q, from Sigma_z (sz6: its
// lower triangle, the identity beyond m), Q (q6: zero beyond m) and nu, all row-uniform -- and what it reports beside the scores
template <class T> struct RobustScale {
    T lam, d0sq;   // lambda (1 for a row that is not inflated) and the raw distance d^2(1)
    int its;       // Newton steps taken
    bool accept;   // the engine's gate, which acts on d0sq
};
template <class T, class A>
UKFB_DEV RobustScale<T> robust_scale(const A& a, const T (&sz6)[6], const T (&q6)[6], const T (&nu)[3], int m, bool eligible);

// true for the argument struct of ukf_robust_kernel (ukf_robust.hpp)
template <class A> inline constexpr bool sensor_args_robust = false;

// The body is ukf_sensor_meas_body.inc.hpp, included in the kernel: the robust update (ukf_robust.hpp) runs it too.
template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_sensor_meas_kernel(const SensorArgs<T, TS> a) {
#include "ukf_sensor_meas_body.inc.hpp"
}

}  // namespace ukfb
