/* ukf_batch_delayed_sensor.h -- late sensor-frame samples: a delayed lever-arm fix, range or landmark sighting corrects the
 * current state through the history ring.  An extension of ukf_batch.h (same library, same engine handle, same conventions)
 * in a header of its own: ukf_batch.h and the binding's table for it (abi.py) are pinned entry point by entry point, so what is
 * added beside them is declared beside them -- here, and in abi_delayed_sensor.py, which tests/test_delayed_sensor_host.py
 * holds to this header type by type.  Plain C99. */
#ifndef UKF_BATCH_DELAYED_SENSOR_H
#define UKF_BATCH_DELAYED_SENSOR_H

#include "ukf_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A sample of a sensor-frame model (enum ukfb_sensor_model, ids 0 ... 7: ukf_batch.h, "sensor-frame measurements") that was
 * taken `lag` steps ago.  ukfb_update_delayed_dev serves the state-selecting models only; moving a lever-arm fix to the body
 * origin with the PRESENT mean's orientation and feeding its model 0 uses the wrong orientation (the one of step n, not of the
 * sample's step s) and drops the coupling of position and orientation that the sensor-frame h carries through its sigma points.
 * Here h is evaluated on the sigma points of the smoothed past state of step s.
 *
 * The steps are those of ukfb_update_delayed_dev (ukf_batch.h, "late samples", steps 1-5) with one change: in step 3,
 * Z_i = h(X_i) is the sensor-frame h of ukfb_update_sensor_dev, on the measurement space R^m, m = 1 or 3 (no SO(3) model).
 * Everything else is that call's, unchanged: the WINDOW (steps, dt HOST, slots, first_slot, mu_hist_dev, cov_hist_dev, in_a_dev,
 * in_b_dev; step n = steps - 1 is the engine's own state; 1 <= steps <= min(slots, UKFB_DELAYED_MAX_STEPS), more is
 * UKFB_ERR_OUT_OF_RANGE and writes nothing), the LAG (lag_uniform, or lag_dev [capacity] int32; l = 0 is an ordinary sensor-frame
 * update to rounding; l < 0: INACTIVE; l > steps - 1: UKFB_ST_ERR_NEG_DT, the filter keeps every bit; ukfb_delayed_lag_dev gives
 * l from a stamp), the chain's statuses and its refusal of the sample when a chain step fails, the gate (gate_chi2), commit = 0
 * READ-ONLY on the engine, NaN outputs for a filter that commits nothing, the engine's last measurement times (not moved) and
 * the LIMITATION (the ring is not rewritten after a commit: a second late sample for the same filter inside the same window is
 * approximate).
 *
 * MODEL: model_uniform, or model_dev [capacity] (int32) when that pointer is non-NULL; ids are UKFB_SENSOR_*.  A UNIFORM id the
 * engine's model does not have (Pose: 0 ... 4, OrientationState: 5 ... 7) is UKFB_ERR_WRONG_MODEL and writes nothing; a
 * PER-FILTER id that is negative, the other engine's or beyond 7 marks that filter INACTIVE.
 * SAMPLE: z_dev [capacity][3], Q_dev [capacity][9] or one 3 x 3 with q_is_uniform, mount_dev [capacity][7] (r, then qs as x, y, z,
 * w) or NULL: mount_uniform, point_dev [capacity][3] or NULL: point_uniform -- each with the meaning, the table of ids and the
 * rule of reading it has in ukfb_sensor_in.  Inputs a model does not read (z beyond m, Q outside the leading m x m, the unused
 * parts of mount and point, the rotation rate for every model but ORIENT_VELOCITY) are never used and may be NaN; a non-finite
 * value in an entry the filter's model reads is UKFB_ST_ERR_NONFINITE_MEAS.
 * ROTATION RATE of model 5 (UKFB_SENSOR_ORIENT_VELOCITY, h = R(qs)^T (R(q)^T v + (w_gyro - b_g) x r)): w_gyro is the gyro sample
 * AT THE TIME OF THE FIX, taken from the first of
 *   1. rate_dev [capacity][3] (engine precision) when it is non-NULL;
 *   2. in_b_dev, OrientationState's rotation-rate ring, when it is bound and l >= 1: that ring's entry of step s;
 *   3. the engine's latch (the bound input before the latched one, as ukfb_update_sensor_dev reads it).
 * PRECISION: h and the differences Z_i - Z_0, z - Z_0 are evaluated in fp64 in every precision mode, exactly as the sensor-frame
 * kernel does (an fp32 ulp of a beacon tens of metres away is larger than the innovation's resolution); the mean iteration, the
 * deltas and the innovation work on those differences.  Everything else computes as the delayed call: fp32 engines in fp32,
 * with wide_arithmetic in fp64.
 *
 * commit = 1 stores the corrected state, `out` may then be NULL.  Outputs are ukfb_delayed_out itself (device, engine
 * precision, any may be NULL): z_pred [capacity][4] holds the first m entries of z-bar and zeros beyond them, S [capacity][9]
 * (zeros beyond m), innov [capacity][3], maha, loglik [capacity], status [capacity] (uint32), mu_out [capacity][S] / cov_out
 * [capacity][PK]: commit = 0 shows there what commit = 1 would store; they must not be the engine's own arrays or the ring.
 * Status of the call (with commit = 1 also written to the engine's status array): UNINITIALISED; INACTIVE (negative lag, no
 * model); ERR_NEG_DT (out of the window); ERR_NONFINITE_MEAS; ERR_CHOLESKY (any factorisation of the chain, Sigma^s_s, S or
 * Sigma~_n fails); WARN_MEAN_NOCONV; REJECTED_GATE (z_pred, S, innov, maha, loglik are still written); SKIPPED_SMALL_DT /
 * ERR_NEG_DT / ERR_DT_TOO_LARGE of gated dt[c], as an OR over the filter's chain.
 * A filter that commits nothing keeps every bit; it never changes a bit of another filter.  Stream-ordered, joins split
 * streams, no host synchronisation, no allocation at call time (one kernel, no workspace).  Device groups: per shard through
 * ukfb_group_shard.  Not served: bearings, state-block models, the robust and association forms. */
typedef struct ukfb_delayed_sensor_in {
    int steps;                    /* window length, step steps - 1 is the present                                        */
    const double* dt;             /* HOST [steps - 1]                                                                      */
    int slots, first_slot;
    const void* mu_hist_dev;      /* [slots][capacity][S]                                                                  */
    const void* cov_hist_dev;     /* [slots][capacity][PK]                                                                 */
    const void* in_a_dev;         /* [slots][capacity][3] or NULL                                                          */
    const void* in_b_dev;
    int lag_uniform;
    const int32_t* lag_dev;       /* [capacity] or NULL: lag_uniform                                                       */
    int model_uniform;            /* UKFB_SENSOR_*                                                                         */
    const int32_t* model_dev;     /* [capacity] or NULL: model_uniform                                                     */
    const void* z_dev;            /* [capacity][3]  the first m entries are read                                           */
    const void* Q_dev;            /* [capacity][9], or [9] with q_is_uniform                                               */
    int q_is_uniform;
    const void* mount_dev;        /* [capacity][7] r, then qs (x, y, z, w); NULL: mount_uniform                            */
    double mount_uniform[7];
    const void* point_dev;        /* [capacity][3]; NULL: point_uniform                                                    */
    double point_uniform[3];
    const void* rate_dev;         /* [capacity][3] the rotation rate at the time of the sample (model 5), or NULL          */
} ukfb_delayed_sensor_in;
int ukfb_update_delayed_sensor_dev(ukfb_engine* e, const ukfb_delayed_sensor_in* in, int commit, const ukfb_delayed_out* out);
/* Host arrays of doubles, window order, as ukfb_update_delayed: mu_hist [steps][capacity][S], cov_hist [steps][capacity][D][D]
 * (step steps - 1 is not read), in_a / in_b [steps][capacity][3] or NULL; lag [capacity] or NULL (lag_uniform);
 * model_per_filter [capacity] or NULL (then `model`); z [capacity][3], Q [capacity][3][3]; mount [capacity][7] or NULL, then
 * mount_uniform [7] (NULL: r = 0, qs the identity); point [capacity][3] or NULL, then point_uniform [3] (NULL: 0); rate
 * [capacity][3] or NULL.  Outputs (any may be NULL): z_pred [capacity][4], S [capacity][9], innov [capacity][3], maha, loglik,
 * status [capacity], mu_out [capacity][S], cov_out [capacity][D][D].  Synchronises. */
int ukfb_update_delayed_sensor(ukfb_engine* e, int steps, const double* dt, const double* mu_hist, const double* cov_hist,
                               const double* in_a, const double* in_b, int lag_uniform, const int32_t* lag, int model,
                               const int32_t* model_per_filter, const double* z, const double* Q, const double* mount,
                               const double* mount_uniform, const double* point, const double* point_uniform, const double* rate,
                               int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik, uint32_t* status,
                               double* mu_out, double* cov_out);

#ifdef __cplusplus
}
#endif

#endif /* UKF_BATCH_DELAYED_SENSOR_H */
