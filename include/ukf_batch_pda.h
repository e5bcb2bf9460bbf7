/* ukf_batch_pda.h -- probabilistic data association: the sensor-frame update with EVERY gated candidate, each at its posterior
 * association weight.  An extension of ukf_batch.h (same library, same engine handle, same conventions) in a header of its
 * own: ukf_batch.h and the binding's table for it (abi.py) are pinned entry point by entry point, so what is added beside them
 * is declared beside them -- here, and in abi_pda.py, which tests/test_pda_host.py holds to this header type by type.
 * Plain C99. */
#ifndef UKF_BATCH_PDA_H
#define UKF_BATCH_PDA_H

#include "ukf_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ukfb_associate_sensor_dev scores K candidate samples per filter and commits the NEAREST one inside the gate at full weight.
 * For USBL and sonar returns, beacon ranges and landmark fixes in clutter, several candidates inside the gate are the normal
 * case, and a hard pick makes an over-confident filter that locks onto clutter.  The probabilistic data association update
 * (PDAF: Bar-Shalom and Tse) lets every gated candidate contribute with its posterior association weight beta_k, weighs the
 * probability beta_0 that none of them is the target, and widens the covariance by the spread of the weighted innovations.
 *
 * SHARED-H MODE ONLY: ukfb_associate_in is reused with point_per_candidate = 0 (K detections against one hypothesis); a
 * non-zero point_per_candidate is UKFB_ERR_INVALID_ARG (per-hypothesis candidates have different S and K: their combination is
 * a mixture, not PDA).  Models (0 ... 7 of enum ukfb_sensor_model), conventions, the slot layout, the meaning of an ABSENT
 * candidate (a non-finite entry among the first m of its z), the gate cfg.gate_chi2, the commit = 0 READ-ONLY behaviour, stream
 * ordering, no allocation at call time and the fp32 / wide_arithmetic behaviour are those of ukfb_associate_sensor_dev.  Device
 * groups: per shard through ukfb_group_shard.
 *
 * Per filter:
 *   1. steps 1 - 4 of ukfb_update_sensor_dev, once: z-bar, S = Ls Ls^T, Y = C Ls^-T;
 *   2. per candidate nu_k = z_k - z-bar, y_k = Ls^-1 nu_k, d^2_k = |y_k|^2, loglik_k = -0.5 (d^2_k + ln det S + m ln 2 pi):
 *      the numbers the association writes;
 *   3. G = the candidates that are scored and finite and, with gate_chi2 >= 0, have d^2_k <= gate_chi2; n_gated = |G|;
 *   4. WEIGHTS: a_0 = ln lambda_m + ln(1 - P_D P_G,m), a_k = ln P_D + loglik_k for k in G,
 *      A = max a + ln sum exp(a - max a) over {0} and G, beta_0 = exp(a_0 - A), beta_k = exp(a_k - A).  A finite candidate
 *      outside the gate gets beta_k = 0 exactly, a candidate that is not scored NaN.  best = the largest beta (equal weights:
 *      the lower index), that is the nearest candidate inside the gate;
 *   5. y-bar = sum_G beta_k y_k, nu-bar = sum_G beta_k nu_k (innov_comb), P_y = sum_G beta_k y_k y_k^T - y-bar y-bar^T;
 *   6. M = (1 - beta_0) I_m - P_y, Sigma~ = Sigma - Y M Y^T, delta = Y y-bar.  Written out with K = Y Ls^-1:
 *      Sigma~ = beta_0 Sigma + (1 - beta_0) (Sigma - K S K^T) + K (sum beta_k nu_k nu_k^T - nu-bar nu-bar^T) K^T;
 *   7. (mu, Sigma) = applyDelta(mu, Sigma~, delta).
 * The three constants ln lambda_m + ln(1 - P_D P_G,m) (m = 1, m = 3) and ln P_D are formed on the host in double and passed by
 * value.
 * STATUS: UNINITIALISED, INACTIVE, WARN_MEAN_NOCONV and ERR_NONFINITE_MEAS (every candidate absent included) as in the
 * association; ERR_CHOLESKY when Sigma or S fails, or the commit's Sigma~ fails; REJECTED_GATE when some candidate is finite and
 * G is empty: the state is kept bit for bit, beta_0 = 1, every finite beta_k = 0, innov_comb = 0, and the scores are written.
 * A filter that is refused (UNINITIALISED, INACTIVE, ERR_NONFINITE_MEAS, ERR_CHOLESKY) keeps every bit, writes NaN to its float
 * outputs (padding entries of innov and innov_comb: 0) and -1 / 0 to best / n_gated; no filter ever changes a bit of another.
 * ARGUMENT ERRORS, decided on the host before any launch, nothing written: a NULL rule, a rule value outside its range or not
 * finite, P_D P_G >= 1 for either m: UKFB_ERR_INVALID_ARG; candidates outside 1 ... 32: UKFB_ERR_OUT_OF_RANGE; a uniform id of
 * the other engine's models: UKFB_ERR_WRONG_MODEL; the rest as for ukfb_associate_sensor_dev.
 * Out of scope: per-hypothesis candidates; per-candidate or per-filter Q, mount, P_D or lambda; the non-parametric clutter
 * estimate; JPDA or any assignment across filters; bearings on S^2; fusing into the cycle kernels. */
typedef struct ukfb_pda_rule {      /* HOST values, by value */
    double p_detect;                /* P_D, in (0, 1] */
    double p_gate_m1, p_gate_m3;    /* P_G for models with m = 1 / m = 3, in (0, 1]; P_D P_G < 1 */
    double clutter_m1, clutter_m3;  /* lambda: clutter density per unit volume of the measurement space, finite, > 0 */
} ukfb_pda_rule;
typedef struct ukfb_pda_out {       /* device pointers, engine precision; any may be NULL */
    void *z_pred, *S;               /* [capacity][3], [capacity][9]   as ukfb_associate_out with H = 1 */
    void *innov, *maha, *loglik;    /* [candidates][capacity][3], [candidates][capacity] x 2 */
    void *beta;                     /* [candidates][capacity]   association weights */
    void *beta0;                    /* [capacity]               weight of "none of them" */
    void *innov_comb;               /* [capacity][3]            sum_k beta_k nu_k, first m entries (rest 0) */
    int32_t *best, *n_gated;        /* as ukfb_associate_out (best = the largest beta) */
    uint32_t* status;
} ukfb_pda_out;
/* out may be NULL with commit = 1 */
int ukfb_update_pda_dev(ukfb_engine* e, int model_uniform, const ukfb_associate_in* in, const ukfb_pda_rule* rule, int commit,
                        const ukfb_pda_out* out);
/* host arrays of doubles, shaped as for ukfb_associate_sensor in shared-h mode: z [candidates][capacity][3], point [capacity][3]
 * or NULL; beta [candidates][capacity], beta0 [capacity], innov_comb [capacity][3]: any output may be NULL.  Synchronises. */
int ukfb_update_pda(ukfb_engine* e, int model, const int32_t* model_per_filter, int candidates, const double* z, const double* Q,
                    const double* mount, const double* mount_uniform, const double* point, const double* point_uniform,
                    const ukfb_pda_rule* rule, int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik,
                    double* beta, double* beta0, double* innov_comb, int32_t* best, int32_t* n_gated, uint32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* UKF_BATCH_PDA_H */
