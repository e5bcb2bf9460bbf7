/* ukf_batch_relative.h -- relative measurements: odometry and scan-match increments between two steps.  An extension of
 * ukf_batch.h (same library, same engine handle, same conventions) in a header of its own: ukf_batch.h and the binding's table
 * for it (abi.py) are pinned entry point by entry point, so what is added beside them is declared beside them -- here, and in
 * abi_relative.py, which tests/test_relative_host.py holds to this header type by type.  Plain C99. */
#ifndef UKF_BATCH_RELATIVE_H
#define UKF_BATCH_RELATIVE_H

#include "ukf_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An INCREMENT "since step s you moved by dp and turned by dq" (wheel or DVL odometry, ICP scan matching, visual odometry)
 * corrects the current state.  Composing it onto the stored mean of step s and feeding an absolute pose counts the uncertainty
 * of step s twice and drops its correlation with the present; here the measurement is made on the PAIR (x_n, x_s): ukfom's
 * update on the state augmented by a clone of step s (stochastic cloning), of which only the present state is kept.  The clone
 * is not carried by the filter: the delayed update's backward chain recovers it from the history ring.  Pose engines only.
 *
 * WINDOW, LAG: ukfb_update_delayed_dev's, field for field (steps, dt HOST, slots, first_slot, mu_hist_dev, cov_hist_dev, in_a_dev,
 * in_b_dev; step n = steps - 1 is the engine's own state; 1 <= steps <= min(slots, UKFB_DELAYED_MAX_STEPS), more is
 * UKFB_ERR_OUT_OF_RANGE and writes nothing).  The increment spans step s = n - l to the present: lag_uniform or lag_dev.
 * l <= 0: INACTIVE -- an increment over no steps measures nothing.  l > steps - 1: UKFB_ST_ERR_NEG_DT, the filter keeps every
 * bit.  ukfb_delayed_lag_dev gives l from the stamp of the increment's START.
 * MODEL (model_uniform, or model_dev [capacity] int32; any other id: INACTIVE):
 *   UKFB_RELATIVE_POSE      m = 6   (R(q_s)^T (p_n - p_s), q_s^-1 q_n)   on R^3 x SO(3)
 *   UKFB_RELATIVE_POSITION  m = 3    R(q_s)^T (p_n - p_s)
 *   UKFB_RELATIVE_ROTATION  m = 3    q_s^-1 q_n                          on SO(3)
 * SAMPLE: z_dev [capacity][7] = dp[3], then dq as x, y, z, w -- the quaternion is taken as given, as the state's is (q^-1 is
 * conj(q) / |q|^2).  A model reads only its own part; the rest may hold anything, NaN included.  Q_dev [capacity][36], or one
 * 6 x 6 with q_is_uniform: row-major in the tangent order (dp, dtheta), dtheta the right perturbation dq exp(dtheta); the lower
 * triangle of the rows and columns the model selects is read.
 * MOUNT: a sensor that is not at the body origin is the caller's: for a relative pose the conjugation z_body = T_m z_sensor
 * T_m^-1 (T_m = (r, q_m) the sensor's pose in the body frame) involves no state, so it is done once on the sample:
 * dq_body = q_m dq q_m^-1, dp_body = R(q_m) dp + r - R(dq_body) r; Q goes with it as Q_body = A Q A^T, A the Jacobian of that
 * map in the tangent order above (rotation block R(q_m), position block R(q_m), and R(dq_body) [r]x R(q_m) from dtheta to dp).
 * ORIENTATIONSTATE ENGINES return UKFB_ERR_WRONG_MODEL.  The conditional covariance of the clone, Sigma_e below, is formed from
 * the chain's first-order transports: on the project's hot histories its smallest correlation-scaled eigenvalue is 6.9e-5 for
 * Pose (lag 1), but 4.7e-11 for OrientationState, and -1.4e-6 for one filter at lag 5 -- negative beyond rounding, so that the
 * joint covariance of the pair is not one.
 *
 * Per filter (D = 12):
 *   1. steps 1-2 of ukfb_update_delayed_dev unchanged: (mu^s_s, Sigma^s_s), M_s with Cov(x_s, x_n) = M_s Sigma_n, and the
 *      chain's statuses; a broken chain refuses the sample;
 *   2. L_n = chol(Sigma_n); Sigma_e = Sigma^s_s - M_s Sigma_n M_s^T (lower triangle) = L_e L_e^T by the CLAMPED rule: with x_k
 *      the pivot after its subtractions, a_kk the entry of Sigma^s_s and tau = 64 eps of the arithmetic the kernel computes in,
 *      x_k > tau a_kk is an ordinary column, |x_k| <= tau a_kk a zero column (that direction of the clone is determined by the
 *      present: a small process noise makes Sigma_e singular to rounding by construction), x_k < -tau a_kk is ERR_CHOLESKY.
 *      The scale is the entry of Sigma^s_s, the minuend, and not Sigma_e's own: in a determined direction Sigma_e's entry is
 *      the rounding error of the subtraction, of either sign (zero process noise on a block: -2e-18 beside a_kk = 4e-2).
 *      (L_n, 0; M_s L_n, L_e) is the lower Cholesky factor of the joint covariance of (x_n, x_s) wherever no pivot is clamped;
 *   3. 4 D + 1 sigma-point pairs: (mu_n, mu^s_s); for j < D (mu_n (+) +-L_n col j, mu^s_s (+) +-(M_s L_n) col j); then
 *      (mu_n, mu^s_s (+) +-L_e col j); Z_i = h(X_n,i, X_s,i);
 *   4. z-bar = the iterated mean on the measurement manifold from Z_0, weight 1 / (4 D + 1) (mean_tol, mean_max_iter);
 *      S = 1/2 sum dz dz^T + Q[sel][sel]; C_n = sum_j (L_n col j) W_j^T, W_j = 1/2 (dz_j+ - dz_j-) over the first 2 D points
 *      only; S = Ls Ls^T, Y_n = C_n Ls^-T, nu = z (-) z-bar, y = Ls^-1 nu, d^2 = |y|^2, ln det S, loglik with m ln 2 pi; the
 *      gate is ukfb_update_dev's (gate_chi2);
 *   5. Sigma~_n = Sigma_n - Y_n Y_n^T, (mu_n, Sigma_n) <- applyDelta(mu_n, Sigma~_n, Y_n y).  The clone is dropped.
 *
 * commit = 0 is READ-ONLY on the engine; commit = 1 stores the corrected state, `out` may then be NULL.  Outputs (device,
 * engine precision, any may be NULL): z_pred [capacity][7], S [capacity][36], innov [capacity][6] (entries outside the model's
 * part are 0), maha, loglik [capacity], status [capacity] (uint32), mu_out [capacity][S] / cov_out [capacity][PK]: commit = 0
 * shows there what commit = 1 would store; they must not be the engine's own arrays or the ring.
 * Status of the call (with commit = 1 also written to the engine's status array): UNINITIALISED; INACTIVE (lag <= 0, no model);
 * ERR_NEG_DT (out of the window); ERR_NONFINITE_MEAS (an entry of z or Q that the model reads); ERR_CHOLESKY (any factorisation
 * of the chain, Sigma_n, Sigma_e, S or Sigma~_n fails); WARN_MEAN_NOCONV; REJECTED_GATE (the scores are still written);
 * SKIPPED_SMALL_DT / ERR_NEG_DT / ERR_DT_TOO_LARGE of gated dt[c], as an OR over the filter's chain.
 * A filter that commits nothing keeps every bit and gets NaN in its float outputs; it never changes a bit of another filter.
 * Stream-ordered, joins split streams, no host synchronisation, no allocation at call time (one kernel, no workspace); fp32
 * engines compute in fp32, with wide_arithmetic in fp64.  Device groups: per shard through ukfb_group_shard.  The ring is not
 * rewritten after a commit (the delayed update's LIMITATION). */
enum ukfb_relative_model { UKFB_RELATIVE_NONE = -1,
    UKFB_RELATIVE_POSE = 0,      /* m = 6  (R(q_s)^T (p_n - p_s),  q_s^-1 q_n)  on R^3 x SO(3) */
    UKFB_RELATIVE_POSITION = 1,  /* m = 3   R(q_s)^T (p_n - p_s)                               */
    UKFB_RELATIVE_ROTATION = 2   /* m = 3   q_s^-1 q_n                           on SO(3)      */ };
typedef struct ukfb_relative_in {
    int steps;                    /* window length, step steps - 1 is the present                                        */
    const double* dt;             /* HOST [steps - 1]                                                                      */
    int slots, first_slot;
    const void* mu_hist_dev;      /* [slots][capacity][S]                                                                  */
    const void* cov_hist_dev;     /* [slots][capacity][PK]                                                                 */
    const void* in_a_dev;         /* [slots][capacity][3] or NULL                                                          */
    const void* in_b_dev;
    int lag_uniform;
    const int32_t* lag_dev;       /* [capacity] or NULL: lag_uniform                                                       */
    int model_uniform;
    const int32_t* model_dev;     /* [capacity] or NULL: model_uniform                                                     */
    const void* z_dev;            /* [capacity][7]                                                                         */
    const void* Q_dev;            /* [capacity][36], or [36] with q_is_uniform                                             */
    int q_is_uniform;
} ukfb_relative_in;
typedef struct ukfb_relative_out { /* device pointers, engine precision; any may be NULL                                   */
    void* z_pred;                 /* [capacity][7]                                                                         */
    void* S;                      /* [capacity][36]                                                                        */
    void* innov;                  /* [capacity][6]                                                                         */
    void* maha;                   /* [capacity]                                                                            */
    void* loglik;                 /* [capacity]                                                                            */
    uint32_t* status;             /* [capacity]                                                                            */
    void* mu_out;                 /* [capacity][S]                                                                         */
    void* cov_out;                /* [capacity][PK]                                                                        */
} ukfb_relative_out;
int ukfb_update_relative_dev(ukfb_engine* e, const ukfb_relative_in* in, int commit, const ukfb_relative_out* out);
/* Host arrays of doubles, window order, as ukfb_update_delayed: mu_hist [steps][capacity][S], cov_hist [steps][capacity][D][D]
 * (step steps - 1 is not read), in_a / in_b [steps][capacity][3] or NULL; lag [capacity] or NULL (lag_uniform);
 * model_per_filter [capacity] or NULL; z [capacity][7], Q [capacity][6][6].  Outputs (any may be NULL): z_pred [capacity][7],
 * S [capacity][36], innov [capacity][6], maha, loglik, status [capacity], mu_out [capacity][S], cov_out [capacity][D][D].
 * Synchronises. */
int ukfb_update_relative(ukfb_engine* e, int steps, const double* dt, const double* mu_hist, const double* cov_hist, const double* in_a,
                         const double* in_b, int lag_uniform, const int32_t* lag, int model, const int32_t* model_per_filter,
                         const double* z, const double* Q, int commit, double* z_pred, double* S, double* innov, double* maha,
                         double* loglik, uint32_t* status, double* mu_out, double* cov_out);

#ifdef __cplusplus
}
#endif

#endif /* UKF_BATCH_RELATIVE_H */
