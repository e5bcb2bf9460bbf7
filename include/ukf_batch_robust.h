/* ukf_batch_robust.h -- the robust sensor-frame update: outliers are down-weighted, not rejected.  An extension of ukf_batch.h
 * (same library, same engine handle, same conventions) in a header of its own: ukf_batch.h and the binding's table for it
 * (abi.py) are pinned entry point by entry point, so what is added beside them is declared beside them -- here, and in
 * abi_robust.py, which tests/test_robust_host.py holds to this header type by type.  Plain C99. */
#ifndef UKF_BATCH_ROBUST_H
#define UKF_BATCH_ROBUST_H

#include "ukf_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The sensor-frame measurements (ukfb_update_sensor_dev, models 0 ... 7 of enum ukfb_sensor_model) serve sensors whose samples
 * are unreliable: USBL and sonar fixes, beacon ranges, DVL velocities, magnetometers.  The hard gate cfg.gate_chi2 takes a
 * sample at full weight or drops it whole: a slightly over-confident filter then rejects every following fix and never
 * recovers, and a filter with the gate off swallows a multipath return at full weight.  The M-estimator update between the
 * two: a sample whose Mahalanobis distance exceeds a threshold c^2 is still used, but its noise covariance is inflated by a
 * scalar lambda >= 1, so that the update it makes is bounded.  A robust update with scale lambda IS ukfb_update_sensor_dev
 * with lambda Q.
 *
 * Inputs (ukfb_sensor_in), models, conventions, the commit = 0 READ-ONLY behaviour, stream ordering, no allocation at call time
 * and the fp32 / wide_arithmetic behaviour are those of ukfb_update_sensor_dev.  Device groups: per shard through
 * ukfb_group_shard.
 *
 * Per filter:
 *   1. steps 1 - 3 of ukfb_update_sensor_dev unchanged: z-bar, Sigma_z = 1/2 sum dz dz^T, C and nu = z - z-bar.  Q is kept
 *      apart from Sigma_z;
 *   2. S(lambda) = Sigma_z + lambda Q on the leading m x m block, d^2(lambda) = nu^T S(lambda)^-1 nu, and the RAW distance
 *      d0^2 = d^2(1).  S(1) not positive definite: ERR_CHOLESKY, as in ukfb_update_sensor_dev;
 *   3. GATE: the engine's own gate acts on the raw distance.  gate_chi2 >= 0 and d0^2 > gate_chi2: REJECTED_GATE, the state is
 *      kept, the scores are written for lambda = 1 with iterations = 0.  With c^2 that gives three zones: full weight,
 *      reduced weight, rejected;
 *   4. INLIERS: c^2 = chi2_m1 or chi2_m3 by the model's m.  d0^2 <= c^2: lambda = 1, iterations = 0, and every number of
 *      the call is ukfb_update_sensor_dev's;
 *   5. UKFB_ROBUST_HUBER, d0^2 > c^2: lambda = sqrt(d0^2 / c^2).  One evaluation, no loop;
 *   6. UKFB_ROBUST_MATCH, d0^2 > c^2: lambda is the root of d^2(lambda) = c^2, which is unique: d^2 falls strictly in lambda
 *      for positive definite Q.  NEWTON on psi(lambda) = 1 / d^2(lambda) - 1 / c^2 from lambda = 1: with x = S(lambda)^-1 nu,
 *      f = nu^T x and g = x^T Q x the step is lambda <- lambda + f (f - c^2) / (c^2 g).  psi is concave and increasing (1 / psi
 *      is a weighted harmonic mean of the shifted generalised eigenvalues of (Sigma_z, Q)), so the iterates rise MONOTONICALLY
 *      towards the root and never pass it -- in exact arithmetic.  In the engine's precision f carries a relative rounding
 *      error of a few eps cond(S(lambda)) (S scaled to a unit diagonal), and the returned lambda may lie past the root by
 *      that much: d^2(lambda) >= c^2 (1 - e), e of that size, is what tests/test_gpu_score_primitives.py holds.  For m = 1, or
 *      Sigma_z proportional to Q, one step is exact.  With tol below that rounding error a filter ends on the rounded f
 *      meeting tol or on a step that no longer increases lambda, not on the cap.  A filter stops on the
 *      first of: f - c^2 <= tol c^2; a step that does not increase lambda; g not positive or not finite; a pivot of S(lambda)
 *      that fails; lambda >= scale_max; max_iter steps.  There is no status bit for the cap: iterations == max_iter together
 *      with maha > c^2 (1 + tol) is how a caller sees it;
 *   7. lambda <- min(lambda, scale_max); steps 4 - 7 of ukfb_update_sensor_dev on S(lambda): Ls, Y = C Ls^-T, y, Sigma~ =
 *      Sigma - Y Y^T and applyDelta.
 * Status of the call: ukfb_update_sensor_dev's; ERR_CHOLESKY also covers the final S(lambda).  A filter that is refused
 * (UNINITIALISED, INACTIVE, ERR_NONFINITE_MEAS, ERR_CHOLESKY) keeps every bit, writes NaN to its float outputs (scale
 * included) and 0 to iterations, and never changes a bit of another filter.
 * ARGUMENT ERRORS: a NULL rule, an unknown mode, a rule value that is not finite or out of its range: UKFB_ERR_INVALID_ARG,
 * decided on the host before any launch; the other arguments as for ukfb_update_sensor_dev.
 * Out of scope: per-component or matrix-valued weights, Student-t rules, robust forms of the other updates. */
enum ukfb_robust_mode { UKFB_ROBUST_MATCH = 0, UKFB_ROBUST_HUBER = 1 };
typedef struct ukfb_robust_rule {   /* HOST values, by value */
    int    mode;
    double chi2_m1, chi2_m3;   /* threshold c^2 for models with m = 1 / m = 3: finite, > 0          */
    double scale_max;          /* lambda is clamped to [1, scale_max]: finite, >= 1                 */
    double tol;                /* MATCH: stop when d^2(lambda) - c^2 <= tol c^2: finite, >= 0       */
    int    max_iter;           /* MATCH: cap on Newton steps, 1 ... 64                              */
} ukfb_robust_rule;
typedef struct ukfb_robust_out {    /* device pointers, engine precision; any may be NULL */
    void *z_pred, *S, *innov;       /* as ukfb_sensor_out; S = Sigma_z + lambda Q                   */
    void *maha0;                    /* [capacity] d0^2 = d^2(1), the raw distance                   */
    void *maha, *loglik;            /* [capacity] d^2(lambda), -0.5 (d^2(lambda) + ln det S(lambda) + m ln 2 pi) */
    void *scale;                    /* [capacity] lambda                                            */
    int32_t*  iterations;           /* [capacity] Newton steps taken (HUBER: 0)                     */
    uint32_t* status;
} ukfb_robust_out;
/* out may be NULL with commit = 1 */
int ukfb_update_robust_dev(ukfb_engine* e, int model_uniform, const ukfb_sensor_in* in, const ukfb_robust_rule* rule, int commit,
                           const ukfb_robust_out* out);
/* host arrays of doubles, shaped as for ukfb_update_sensor; maha0, maha, loglik, scale, iterations (int32), status [capacity]:
 * any output may be NULL.  Synchronises. */
int ukfb_update_robust(ukfb_engine* e, int model, const int32_t* model_per_filter, const double* z, const double* Q,
                       const double* mount, const double* mount_uniform, const double* point, const double* point_uniform,
                       const ukfb_robust_rule* rule, int commit, double* z_pred, double* S, double* innov, double* maha0,
                       double* maha, double* loglik, double* scale, int32_t* iterations, uint32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* UKF_BATCH_ROBUST_H */
