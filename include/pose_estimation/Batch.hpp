// pose_estimation/Batch.hpp -- batched C++ siblings of PoseUKF / OrientationUKF: one object owns N
// filters resident on one MI355X.  Thin RAII over include/ukf_batch.h; arrays are AoS doubles in the
// layouts documented there.  This is the interface the engine is built for (a Rock component that
// tracks N hypotheses / particles / vehicles calls these instead of N scalar objects).
#ifndef _POSE_ESTIMATION_BATCH_HPP
#define _POSE_ESTIMATION_BATCH_HPP

#include <ukf_batch.h>
#include <ukf_batch_relative.h>
#include <ukf_batch_robust.h>
#include <ukf_batch_pda.h>
#include <ukf_batch_assign.h>
#include <ukf_batch_jpda.h>
#include <ukf_batch_delayed_sensor.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace pose_estimation
{

class BatchUKF
{
public:
    BatchUKF(int model, int precision, int64_t capacity, int device = 0, void* hip_stream = NULL) : engine(NULL)
    {
        if (ukfb_create(&engine, model, precision, capacity, device, hip_stream) != UKFB_OK)
            throw std::runtime_error(std::string("pose_estimation: MI355X engine unavailable: ") + ukfb_last_error());
        ukfb_describe(engine, NULL, NULL, &cap, &S, &D, &PK);
    }
    virtual ~BatchUKF() { ukfb_destroy(engine); }

    int64_t capacity() const { return cap; }
    int storedSize() const { return S; }
    int dof() const { return D; }
    ukfb_engine* handle() { return engine; }

    /** initializeFilter for filters [first, first + count) */
    virtual void initializeFilters(int64_t first, int64_t count, const double* mu, const double* cov) { check(ukfb_initialize(engine, first, count, mu, cov)); }
    /** getCurrentState for filters [first, first + count); cov may be NULL */
    void getCurrentStates(int64_t first, int64_t count, double* mu, double* cov, uint8_t* initialised = NULL) { check(ukfb_get_state(engine, first, count, mu, cov, initialised)); }
    void setProcessNoiseCovariance(const double* R) { check(ukfb_set_process_noise(engine, R)); }
    void setProcessNoiseCovariances(int64_t first, int64_t count, const double* R) { check(ukfb_set_process_noise_per_filter(engine, first, count, R)); }
    void setLastMeasurementTimes(int64_t first, int64_t count, const int64_t* t_us) { check(ukfb_set_last_measurement_time(engine, first, count, t_us)); }
    void setTimeDeltas(double min_dt, double max_dt)
    {
        ukfb_config c; ukfb_get_config(engine, &c); c.min_time_delta = min_dt; c.max_time_delta = max_dt; check(ukfb_set_config(engine, &c));
    }
    /** predictionStep(delta_t) for every filter; per-filter outcomes in status() */
    void predictionStep(double delta_t) { check(ukfb_predict(engine, delta_t)); }
    void predictionSteps(const double* delta_t) { check(ukfb_predict_dt(engine, delta_t)); }
    /** predictionStepFromSampleTime(ts[i]) per filter (int64 microseconds) */
    void predictionStepsFromSampleTimes(const int64_t* ts_us) { check(ukfb_predict_timestamps(engine, ts_us)); }
    /** integrateMeasurement with one model id (UKFB_MEAS_*) for the batch */
    void integrateMeasurements(int model, const double* z, const double* Q, const uint8_t* active = NULL) { check(ukfb_update(engine, model, z, Q, active)); }
    /** per-filter model ids (negative = none): the asynchronous mixed stream of BASELINE config 5 */
    void integrateMixedMeasurements(const int32_t* model, const double* z, const double* Q) { check(ukfb_update_mixed(engine, model, z, Q)); }
    /** fused predictionStep + integrateMeasurement in one launch */
    void cycle(double delta_t, int model, const double* z, const double* Q) { check(ukfb_cycle(engine, delta_t, model, z, Q)); }
    /** `cycles` fused cycles in one launch, the filters stay on chip in between: buffered fixed-rate samples, one input set
     *  per cycle (z [cycles][N][3], Q [cycles][N][9]; in_a / in_b [cycles][N][3] or NULL = the latched inputs).
     *  Pose: in_a = acceleration; Orient: in_a = acceleration, in_b = rotation rate */
    void cycles(int cycles, double delta_t, int model, const double* in_a, const double* in_b, const double* z, const double* Q)
    {
        check(ukfb_cycle_multi(engine, cycles, delta_t, model, in_a, in_b, z, Q));
    }
    /** fused predictionStepFromSampleTime(ts[i]) + integrateMeasurement(model[i]); ts < 0: no sample, model < 0: predict only */
    void cycleFromSampleTimes(const int64_t* ts_us, const int32_t* model, const double* z, const double* Q) { check(ukfb_cycle_timestamps(engine, ts_us, model, z, Q)); }
    /** time-ordered asynchronous stream of samples in any arrival order (the batched stream aligner); returns the number of launches */
    int64_t processEvents(int64_t n_events, const int64_t* filter, const int64_t* ts_us, const int32_t* model, const double* z, const double* Q)
    {
        int64_t rounds = 0;
        check(ukfb_process_events(engine, n_events, filter, ts_us, model, z, Q, NULL, &rounds));
        return rounds;
    }
    /** Innovation statistics WITHOUT an update (ukfb_innovation): `candidates` samples per filter, z [candidates][N][3],
     *  Q [N][3][3].  The filters are not changed.  With maha a caller evaluates any acceptance predicate ukfom allows;
     *  best is the nearest candidate inside ukfb_config.gate_chi2 (-1: none). */
    struct Innovation
    {
        std::vector<double> z_pred;    // [N][4]
        std::vector<double> S;         // [N][3][3]
        std::vector<double> innov;     // [candidates][N][3]
        std::vector<double> maha;      // [candidates][N]
        std::vector<double> loglik;    // [candidates][N]
        std::vector<int32_t> best;     // [N]
        std::vector<uint32_t> status;  // [N]  UKFB_ST_* of the call
    };
    Innovation innovation(int model, int candidates, const double* z, const double* Q)
    {
        const size_t n = static_cast<size_t>(cap), k = static_cast<size_t>(candidates > 0 ? candidates : 0);
        Innovation r;
        r.z_pred.resize(n * 4); r.S.resize(n * 9); r.innov.resize(k * n * 3); r.maha.resize(k * n); r.loglik.resize(k * n);
        r.best.resize(n); r.status.resize(n);
        check(ukfb_innovation(engine, model, candidates, z, Q, r.z_pred.data(), r.S.data(), r.innov.data(), r.maha.data(),
                              r.loglik.data(), r.best.data(), r.status.data()));
        return r;
    }
    /** nearest-neighbour association from host arrays: z_sel [N][3] = the chosen candidate of every filter, model_sel [N] = model
     *  or -1 where best < 0 -- the arguments of integrateMixedMeasurements(model_sel, z_sel, Q) */
    void selectCandidates(int model, int candidates, const std::vector<int32_t>& best, const double* z, std::vector<double>& z_sel,
                          std::vector<int32_t>& model_sel) const
    {
        const size_t n = static_cast<size_t>(cap);
        if (best.size() != n) throw std::runtime_error("pose_estimation engine: selectCandidates needs one choice per filter");
        z_sel.assign(n * 3, 0.0);
        model_sel.assign(n, -1);
        for (size_t i = 0; i < n; ++i) {
            if (best[i] < 0 || best[i] >= candidates) continue;
            for (int c = 0; c < 3; ++c) z_sel[i * 3 + c] = z[(static_cast<size_t>(best[i]) * n + i) * 3 + c];
            model_sel[i] = model;
        }
    }
    /** Filter banks (ukf_batch.h, "filter banks"): the batch read as capacity / hypotheses tracks of `hypotheses` filters each,
     *  track-major.  bankCombine: the mixture moments of every track under the weights w [N] (the filters are not changed). */
    struct BankEstimate
    {
        std::vector<double> mu;        // [T][S]
        std::vector<double> cov;       // [T][D][D]
        std::vector<uint32_t> status;  // [T]  UKFB_ST_* of the call
    };
    BankEstimate bankCombine(int hypotheses, const double* w)
    {
        const size_t t = hypotheses > 0 ? static_cast<size_t>(cap) / static_cast<size_t>(hypotheses) : 0;
        BankEstimate r;
        r.mu.resize(t * S); r.cov.resize(t * D * D); r.status.resize(t);
        check(ukfb_bank_combine(engine, hypotheses, w, r.mu.data(), r.cov.data(), r.status.data()));
        return r;
    }
    /** IMM interaction: every hypothesis re-seeded from all of its track under the row-stochastic transition [M][M]; returns the
     *  predicted model probabilities [N]; status [T] (may be NULL) receives the per-track status of the call */
    std::vector<double> bankMix(int hypotheses, const double* w, const double* transition, std::vector<uint32_t>* status = NULL)
    {
        const size_t t = hypotheses > 0 ? static_cast<size_t>(cap) / static_cast<size_t>(hypotheses) : 0;
        std::vector<double> w_pred(static_cast<size_t>(cap));
        if (status) status->assign(t, 0u);
        check(ukfb_bank_mix(engine, hypotheses, w, transition, w_pred.data(), status ? status->data() : NULL));
        return w_pred;
    }
    /** posterior weights on the device (engine precision arrays [N]): logw_out = logw_in + loglik - logsumexp per track */
    void bankWeights(int hypotheses, const void* logw_in_dev, const void* loglik_dev, void* logw_out_dev, void* w_out_dev = NULL,
                     uint32_t* status_dev = NULL)
    {
        check(ukfb_bank_weights_dev(engine, hypotheses, logw_in_dev, loglik_dev, logw_out_dev, w_out_dev, status_dev));
    }
    /** Fixed-interval smoothing (ukf_batch.h, "fixed-interval smoothing").  historyPush: stream-ordered copy of the current
     *  mean and packed covariance into slot `slot` of the caller's device rings [slots][N][S] / [slots][N][PK]. */
    void historyPush(int slots, int slot, void* mu_hist_dev, void* cov_hist_dev)
    {
        check(ukfb_history_push_dev(engine, slots, slot, mu_hist_dev, cov_hist_dev));
    }
    /** the RTS backward pass over `steps` slots from first_slot on; dt: host, steps - 1 entries; outputs: rings like the history
     *  (they may be the history itself; cov_out_dev may be NULL); in_a_dev / in_b_dev: input rings or NULL (the latched inputs) */
    void smoothDev(int steps, const double* dt, int slots, int first_slot, const void* mu_hist_dev, const void* cov_hist_dev,
                   void* mu_out_dev, void* cov_out_dev = NULL, uint32_t* status_dev = NULL, const void* in_a_dev = NULL,
                   const void* in_b_dev = NULL)
    {
        check(ukfb_smooth_dev(engine, steps, dt, slots, first_slot, mu_hist_dev, cov_hist_dev, in_a_dev, in_b_dev, mu_out_dev,
                              cov_out_dev, status_dev));
    }
    /** Joint state-block measurements (ukf_batch.h, "joint state-block measurements"): ukf->update(z, h, Q) with z the compound
     *  of the blocks `block_mask` selects (UKFB_BLOCK_*) and h their selection.  Device form: z_dev [N][S] in the state's own
     *  layout, Qz_packed_dev [N][PK] (a record of deviceViews, a history slot or bankCombineDev as it lies); block_mask_dev
     *  int32 [N] or NULL; the update runs on state_inflation * Sigma and meas_inflation * Qz (1 / w, 1 / (1 - w): covariance
     *  intersection); commit = false is read-only (only `out` is written).  Stream-ordered. */
    void integrateStateMeasurementsDev(uint32_t block_mask, const void* z_dev, const void* Qz_packed_dev,
                                       const int32_t* block_mask_dev = NULL, double state_inflation = 1.0,
                                       double meas_inflation = 1.0, bool commit = true, const ukfb_state_meas_out* out = NULL)
    {
        check(ukfb_update_state_dev(engine, block_mask, block_mask_dev, z_dev, Qz_packed_dev, state_inflation, meas_inflation,
                                    commit ? 1 : 0, out));
    }
    /** host arrays: z [N][S], Qz [N][D][D], block_mask_per_filter [N] or NULL; maha / loglik [N] or NULL; returns the status */
    std::vector<uint32_t> integrateStateMeasurements(uint32_t block_mask, const double* z, const double* Qz,
                                                     const int32_t* block_mask_per_filter = NULL, double state_inflation = 1.0,
                                                     double meas_inflation = 1.0, bool commit = true, double* maha = NULL,
                                                     double* loglik = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_state(engine, block_mask, block_mask_per_filter, z, Qz, state_inflation, meas_inflation, commit ? 1 : 0,
                                maha, loglik, st.data()));
        return st;
    }
    /** Sensor-frame measurements (ukf_batch.h, "sensor-frame measurements"): ukf->update(z, h, Q) with h one of the
     *  UKFB_SENSOR_* models -- a lever arm, a range, a point seen in the sensor frame, a velocity at the sensor, a nav-frame
     *  vector -- so that the sigma points carry the coupling to the orientation and angular-velocity uncertainty that shifting
     *  the sample into the body frame with the current mean discards.  Device form: the arrays of ukfb_sensor_in; commit =
     *  false is read-only (only `out` is written).  Stream-ordered. */
    void integrateSensorMeasurementDev(int model_uniform, const ukfb_sensor_in& in, bool commit = true, const ukfb_sensor_out* out = NULL)
    {
        check(ukfb_update_sensor_dev(engine, model_uniform, &in, commit ? 1 : 0, out));
    }
    /** host arrays: z [N][3], Q [N][3][3]; mount_uniform [7] = r, then qs (x, y, z, w) (NULL: r = 0, qs the identity) and
     *  point_uniform [3] (NULL: 0) serve every filter unless mount [N][7] / point [N][3] are given; model_per_filter [N] or
     *  NULL; z_pred [N][3], S [N][3][3], innov [N][3], maha / loglik [N] or NULL; returns the status */
    std::vector<uint32_t> integrateSensorMeasurement(int model, const double* z, const double* Q, const double* mount_uniform = NULL,
                                                     const double* point_uniform = NULL, const double* mount = NULL,
                                                     const double* point = NULL, const int32_t* model_per_filter = NULL,
                                                     bool commit = true, double* z_pred = NULL, double* S = NULL, double* innov = NULL,
                                                     double* maha = NULL, double* loglik = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_sensor(engine, model, model_per_filter, z, Q, mount, mount_uniform, point, point_uniform, commit ? 1 : 0,
                                 z_pred, S, innov, maha, loglik, st.data()));
        return st;
    }
    /** The robust form of the sensor-frame measurements (ukf_batch_robust.h): a sample whose raw Mahalanobis distance exceeds
     *  the rule's threshold is not rejected but updates with lambda Q, lambda >= 1 by the rule's mode; the filters' own gate
     *  acts on the raw distance.  Device form: the arrays of ukfb_sensor_in; commit = false is read-only.  Stream-ordered. */
    void integrateRobustSensorMeasurementDev(int model_uniform, const ukfb_sensor_in& in, const ukfb_robust_rule& rule, bool commit = true,
                                             const ukfb_robust_out* out = NULL)
    {
        check(ukfb_update_robust_dev(engine, model_uniform, &in, &rule, commit ? 1 : 0, out));
    }
    /** host arrays, shaped as for integrateSensorMeasurement; maha0 [N] the raw distance, maha [N] the distance under
     *  lambda Q, scale [N] = lambda, iterations [N] the Newton steps taken, or NULL; returns the status */
    std::vector<uint32_t> integrateRobustSensorMeasurement(int model, const double* z, const double* Q, const ukfb_robust_rule& rule,
                                                           const double* mount_uniform = NULL, const double* point_uniform = NULL,
                                                           const double* mount = NULL, const double* point = NULL,
                                                           const int32_t* model_per_filter = NULL, bool commit = true,
                                                           double* z_pred = NULL, double* S = NULL, double* innov = NULL,
                                                           double* maha0 = NULL, double* maha = NULL, double* loglik = NULL,
                                                           double* scale = NULL, int32_t* iterations = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_robust(engine, model, model_per_filter, z, Q, mount, mount_uniform, point, point_uniform, &rule, commit ? 1 : 0,
                                 z_pred, S, innov, maha0, maha, loglik, scale, iterations, st.data()));
        return st;
    }
    /** Bearing measurements (ukf_batch.h, "bearing measurements"): ukf->update(z, h, Q) with a direction on the sphere S^2 --
     *  h(X) = d(X) / |d(X)| for one of the UKFB_BEARING_* models, the mean iterated on the sphere, a two-dimensional noise.
     *  The arrays of ukfb_sensor_in with the header's meaning for bearings (z a direction, not necessarily of unit length; Q the
     *  3 x 3 covariance of the direction noise, of which the tangent part enters); commit = false is read-only (only `out` is
     *  written).  Stream-ordered. */
    void integrateBearingMeasurementDev(int model_uniform, const ukfb_sensor_in& in, bool commit = true, const ukfb_sensor_out* out = NULL)
    {
        check(ukfb_update_bearing_dev(engine, model_uniform, &in, commit ? 1 : 0, out));
    }
    /** host arrays, shaped as for integrateSensorMeasurement; z_pred [N][3] the predicted unit vector, S [N][3][3] of rank 2,
     *  innov [N][3] the sphere logarithm; returns the status */
    std::vector<uint32_t> integrateBearingMeasurement(int model, const double* z, const double* Q, const double* mount_uniform = NULL,
                                                      const double* point_uniform = NULL, const double* mount = NULL,
                                                      const double* point = NULL, const int32_t* model_per_filter = NULL,
                                                      bool commit = true, double* z_pred = NULL, double* S = NULL, double* innov = NULL,
                                                      double* maha = NULL, double* loglik = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_bearing(engine, model, model_per_filter, z, Q, mount, mount_uniform, point, point_uniform, commit ? 1 : 0,
                                  z_pred, S, innov, maha, loglik, st.data()));
        return st;
    }
    /** Sensor-frame association (ukf_batch.h, "sensor-frame association"): in.candidates samples per filter scored through a
     *  UKFB_SENSOR_* model in one launch, the nearest candidate inside the gate chosen and, with commit, the update finished
     *  with it.  in.point_per_candidate = 0: every candidate is a detection of the one point; 1: candidate k is a fix of its
     *  own landmark or beacon in.point_dev [candidates][N][3].  commit = false is read-only (only `out` is written).
     *  Stream-ordered. */
    void associateSensorMeasurementDev(int model_uniform, const ukfb_associate_in& in, bool commit = true, const ukfb_associate_out* out = NULL)
    {
        check(ukfb_associate_sensor_dev(engine, model_uniform, &in, commit ? 1 : 0, out));
    }
    /** host arrays: z [candidates][N][3], Q [N][3][3]; mount / point as for integrateSensorMeasurement, with
     *  point_per_candidate point [candidates][N][3]; z_pred [H][N][3], S [H][N][3][3] (H = candidates per hypothesis, else 1),
     *  innov [candidates][N][3], maha / loglik [candidates][N], n_gated [N] or NULL; best [N] receives the chosen candidate
     *  (-1: none); returns the status */
    std::vector<uint32_t> associateSensorMeasurement(int model, int candidates, const double* z, const double* Q, int32_t* best,
                                                     const double* mount_uniform = NULL, const double* point_uniform = NULL,
                                                     const double* mount = NULL, const double* point = NULL,
                                                     bool point_per_candidate = false, const int32_t* model_per_filter = NULL,
                                                     bool commit = true, double* z_pred = NULL, double* S = NULL, double* innov = NULL,
                                                     double* maha = NULL, double* loglik = NULL, int32_t* n_gated = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_associate_sensor(engine, model, model_per_filter, candidates, z, Q, mount, mount_uniform, point, point_uniform,
                                    point_per_candidate ? 1 : 0, commit ? 1 : 0, z_pred, S, innov, maha, loglik, best, n_gated, st.data()));
        return st;
    }
    /** Probabilistic data association (ukf_batch_pda.h): the shared-h association whose update uses EVERY candidate inside the
     *  gate at its posterior association weight beta_k, weighs the probability beta_0 that none is the target, and widens the
     *  covariance by the spread of the weighted innovations.  in.point_per_candidate must be 0; rule: P_D, P_G and the clutter
     *  density for m = 1 / m = 3.  commit = false is read-only (only `out` is written).  Stream-ordered. */
    void integratePdaSensorMeasurementDev(int model_uniform, const ukfb_associate_in& in, const ukfb_pda_rule& rule, bool commit = true,
                                          const ukfb_pda_out* out = NULL)
    {
        check(ukfb_update_pda_dev(engine, model_uniform, &in, &rule, commit ? 1 : 0, out));
    }
    /** host arrays, shaped as for associateSensorMeasurement in shared-h mode; beta [candidates][N] the weights, beta0 [N],
     *  innov_comb [N][3] = sum beta_k nu_k, best / n_gated [N], or NULL; returns the status */
    std::vector<uint32_t> integratePdaSensorMeasurement(int model, int candidates, const double* z, const double* Q, const ukfb_pda_rule& rule,
                                                        const double* mount_uniform = NULL, const double* point_uniform = NULL,
                                                        const double* mount = NULL, const double* point = NULL,
                                                        const int32_t* model_per_filter = NULL, bool commit = true,
                                                        double* z_pred = NULL, double* S = NULL, double* innov = NULL, double* maha = NULL,
                                                        double* loglik = NULL, double* beta = NULL, double* beta0 = NULL,
                                                        double* innov_comb = NULL, int32_t* best = NULL, int32_t* n_gated = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_pda(engine, model, model_per_filter, candidates, z, Q, mount, mount_uniform, point, point_uniform, &rule,
                              commit ? 1 : 0, z_pred, S, innov, maha, loglik, beta, beta0, innov_comb, best, n_gated, st.data()));
        return st;
    }
    /** Global nearest-neighbour assignment (ukf_batch_assign.h): the one-to-one assignment of detections to the filters of
     *  each scene, a contiguous run of slots that share one detection list; in.cost_dev is the maha or -2 loglik an
     *  association call wrote.  out.assign is a drop-in for best_dev.  Read-only on the filters.  Stream-ordered. */
    void assignScenesDev(const ukfb_assign_in& in, const ukfb_assign_out& out) { check(ukfb_assign_scenes_dev(engine, &in, &out)); }
    /** host arrays: cost [candidates][N], scene_start [scenes + 1] (NULL: uniform scenes of tracks_per_scene slots), miss [N]
     *  (NULL: miss_uniform); assign [N], owner [scenes][candidates], objective [scenes], or NULL; returns the scenes' status */
    std::vector<uint32_t> assignScenes(int candidates, const double* cost, int scenes, const int32_t* scene_start, int tracks_per_scene,
                                       double gate, const double* miss, double miss_uniform, int32_t* assign, int32_t* owner = NULL,
                                       double* objective = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(scenes > 0 ? scenes : 0));
        std::vector<uint32_t> none(1);
        check(ukfb_assign_scenes(engine, candidates, cost, scenes, scene_start, tracks_per_scene, gate, miss, miss_uniform, assign, owner,
                                 objective, st.empty() ? none.data() : st.data()));
        return st;
    }
    /** Joint probabilistic data association (ukf_batch_jpda.h): the exact association marginals of each scene (at most six
     *  tracks), from the loglik / maha integratePdaSensorMeasurementDev(commit = false) wrote.  out.beta / out.beta0 may be the
     *  arrays that call filled: bad and too-large scenes keep what is there.  Read-only on the filters.  Stream-ordered. */
    void jpdaScenesDev(const ukfb_jpda_in& in, const ukfb_pda_rule& rule, const ukfb_jpda_out& out) { check(ukfb_jpda_scenes_dev(engine, &in, &rule, &out)); }
    /** host arrays: loglik, maha (or NULL) [candidates][N], scene_start [scenes + 1] (NULL: uniform scenes of tracks_per_scene
     *  slots); beta [candidates][N], beta0 [N], free [scenes][candidates], log_z [scenes], or NULL; returns the scenes' status */
    std::vector<uint32_t> jpdaScenes(int candidates, const double* loglik, const double* maha, int scenes, const int32_t* scene_start,
                                     int tracks_per_scene, double gate, int model, const int32_t* model_per_filter, const ukfb_pda_rule& rule,
                                     double* beta, double* beta0 = NULL, double* free_k = NULL, double* log_z = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(scenes > 0 ? scenes : 0));
        std::vector<uint32_t> none(1);
        check(ukfb_jpda_scenes(engine, candidates, loglik, maha, scenes, scene_start, tracks_per_scene, gate, model, model_per_filter, &rule,
                               beta, beta0, free_k, log_z, st.empty() ? none.data() : st.data()));
        return st;
    }
    /** The probabilistic data association update with GIVEN weights (ukf_batch_jpda.h): weight_dev [candidates][N] in engine
     *  precision, used as w / max(1, sum w); cfg.gate_chi2 plays no part.  commit = false is read-only.  Stream-ordered. */
    void updateWeightedDev(int model_uniform, const ukfb_associate_in& in, const void* weight_dev, bool commit = true,
                           const ukfb_weighted_out* out = NULL)
    {
        check(ukfb_update_weighted_dev(engine, model_uniform, &in, weight_dev, commit ? 1 : 0, out));
    }
    /** host arrays, shaped as for integratePdaSensorMeasurement; weight [candidates][N]; returns the status */
    std::vector<uint32_t> updateWeighted(int model, int candidates, const double* z, const double* Q, const double* weight,
                                         const double* mount_uniform = NULL, const double* point_uniform = NULL, const double* mount = NULL,
                                         const double* point = NULL, const int32_t* model_per_filter = NULL, bool commit = true,
                                         double* z_pred = NULL, double* S = NULL, double* innov = NULL, double* maha = NULL,
                                         double* loglik = NULL, double* weight_used = NULL, double* beta0 = NULL, double* innov_comb = NULL,
                                         int32_t* n_used = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_weighted(engine, model, model_per_filter, candidates, z, Q, mount, mount_uniform, point, point_uniform, weight,
                                   commit ? 1 : 0, z_pred, S, innov, maha, loglik, weight_used, beta0, innov_comb, n_used, st.data()));
        return st;
    }
    /** User-defined measurement models (ukf_batch.h, "user-defined measurement models"): ukf->update(z, h, Q) for an h of the
     *  caller's.  sigmaPointsDev exports every filter's sigma points, filter-major: X_out_dev [N][2 D + 1][S] (point 0 = mu,
     *  1 + 2 j = mu (+) L col j, 2 + 2 j = mu (+) (-L col j)), delta_out_dev [N][2 D + 1][D] the tangent offsets; either may be
     *  NULL, not both; read-only on the filters.  The caller evaluates Z = h(X) and integrateSampledMeasurementDev finishes the
     *  update from in.Z_dev [N][2 D + 1][m], m = 1 ... UKFB_SAMPLED_MAX_M; commit = false is read-only (only `out` is written).
     *  The state must not change between the two calls.  Stream-ordered. */
    void sigmaPointsDev(void* X_out_dev, void* delta_out_dev = NULL, uint32_t* status_dev = NULL)
    {
        check(ukfb_sigma_points_dev(engine, X_out_dev, delta_out_dev, status_dev));
    }
    void integrateSampledMeasurementDev(const ukfb_sampled_in& in, bool commit = true, const ukfb_sampled_out* out = NULL)
    {
        check(ukfb_update_sampled_dev(engine, &in, commit ? 1 : 0, out));
    }
    /** host arrays: X [N][2 D + 1][S], delta [N][2 D + 1][D] (either may be NULL, not both); returns the status */
    std::vector<uint32_t> sigmaPoints(double* X, double* delta = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_sigma_points(engine, X, delta, st.data()));
        return st;
    }
    /** host arrays: Z [N][2 D + 1][m] = h(X) in the order of sigmaPoints, z [N][m], Q [N][m][m] (ONE m x m with q_is_uniform);
     *  active [N] or NULL; z_pred [N][m], S [N][m][m], innov [N][m], maha / loglik [N] or NULL; returns the status */
    std::vector<uint32_t> integrateSampledMeasurement(int m, const double* Z, const double* z, const double* Q,
                                                      bool q_is_uniform = false, const uint8_t* active = NULL, bool commit = true,
                                                      double* z_pred = NULL, double* S = NULL, double* innov = NULL,
                                                      double* maha = NULL, double* loglik = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_sampled(engine, m, Z, z, Q, q_is_uniform ? 1 : 0, active, commit ? 1 : 0, z_pred, S, innov, maha, loglik,
                                  st.data()));
        return st;
    }
    /** User-defined process models (ukf_batch.h, "user-defined process models"): ukf->predict(f, R) for an f of the caller's.
     *  The caller evaluates XX = f(X) on the export of sigmaPointsDev and predictSampledDev finishes the prediction from
     *  in.XX_dev [N][2 D + 1][S] and in.R_dev [N][D][D] (ONE D x D with r_is_uniform; taken as given: no rotation, no dt).
     *  Times are not touched.  commit = false is read-only (only `out` is written).  Stream-ordered. */
    void predictSampledDev(const ukfb_predict_sampled_in& in, bool commit = true, const ukfb_predict_sampled_out* out = NULL)
    {
        check(ukfb_predict_sampled_dev(engine, &in, commit ? 1 : 0, out));
    }
    /** host arrays: XX [N][2 D + 1][S] = f(X) in the order of sigmaPoints, R [N][D][D] (ONE D x D with r_is_uniform); active [N]
     *  or NULL; mu [N][S], cov [N][D][D] or NULL; returns the status */
    std::vector<uint32_t> predictSampled(const double* XX, const double* R, bool r_is_uniform = false, const uint8_t* active = NULL,
                                         bool commit = true, double* mu = NULL, double* cov = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_predict_sampled(engine, XX, R, r_is_uniform ? 1 : 0, active, commit ? 1 : 0, mu, cov, st.data()));
        return st;
    }
    /** Covariance conditioning (ukf_batch.h, "covariance conditioning"): the covariance of every selected filter is judged in its
     *  correlation scaling; one whose smallest correlation eigenvalue is below in.eig_floor / 2, or with a variance below
     *  in.var_floor_dev [D], is repaired where it lives (UKFB_ST_REPAIRED), a healthy one keeps every bit; with
     *  in.renormalize_quaternion the stored quaternion is brought back to unit length.  commit = false is read-only (only `out` is
     *  written).  Stream-ordered. */
    void conditionDev(const ukfb_condition_in& in, bool commit = true, const ukfb_condition_out* out = NULL)
    {
        check(ukfb_condition_dev(engine, &in, commit ? 1 : 0, out));
    }
    /** host arrays: var_floor [D] (finite, > 0), select [N] or NULL; eig_min / eig_max [N], mu [N][S], cov [N][D][D] or NULL;
     *  returns the status */
    std::vector<uint32_t> condition(const double* var_floor, double eig_floor, const uint8_t* select = NULL,
                                    bool renormalize_quaternion = false, bool commit = true, double* eig_min = NULL,
                                    double* eig_max = NULL, double* mu = NULL, double* cov = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_condition(engine, var_floor, eig_floor, select, renormalize_quaternion ? 1 : 0, commit ? 1 : 0, eig_min, eig_max, mu,
                             cov, st.data()));
        return st;
    }
    /** Late samples (ukf_batch.h, "late samples"): a sample taken in.lag steps ago corrects the CURRENT state through the history
     *  ring -- no stored measurements, no replay, no waiting for the slowest sensor.  The window is smoothDev's with the
     *  filters' own state as its last step; commit = false is read-only (only `out` is written, out->mu_out / cov_out showing
     *  what a commit would store).  Stream-ordered. */
    void updateDelayedDev(const ukfb_delayed_in& in, bool commit = true, const ukfb_delayed_out* out = NULL)
    {
        check(ukfb_update_delayed_dev(engine, &in, commit ? 1 : 0, out));
    }
    /** the lag of every filter's sample from its stamp: step_ts_us host [steps], sample_ts_us_dev int64 [N] -> lag_out_dev int32 [N] */
    void delayedLagDev(int steps, const int64_t* step_ts_us, const int64_t* sample_ts_us_dev, int32_t* lag_out_dev)
    {
        check(ukfb_delayed_lag_dev(engine, steps, step_ts_us, sample_ts_us_dev, lag_out_dev));
    }
    /** host arrays in window order: mu_hist [steps][N][S], cov_hist [steps][N][D][D] (the last step is not read), dt [steps - 1],
     *  in_a / in_b [steps][N][3] or NULL; lag / model_per_filter [N] or NULL (lag_uniform / model); z [N][3], Q [N][3][3];
     *  mu_out [N][S] / cov_out [N][D][D] or NULL: the corrected present state.  Returns the status. */
    std::vector<uint32_t> updateDelayed(int steps, const double* dt, const double* mu_hist, const double* cov_hist, int lag_uniform,
                                        int model, const double* z, const double* Q, bool commit = true, const int32_t* lag = NULL,
                                        const int32_t* model_per_filter = NULL, const double* in_a = NULL, const double* in_b = NULL,
                                        double* mu_out = NULL, double* cov_out = NULL, double* maha = NULL, double* loglik = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_delayed(engine, steps, dt, mu_hist, cov_hist, in_a, in_b, lag_uniform, lag, model, model_per_filter, z, Q,
                                  commit ? 1 : 0, NULL, NULL, NULL, maha, loglik, st.data(), mu_out, cov_out));
        return st;
    }
    /** Relative measurements (ukf_batch_relative.h): an odometry or scan-match increment "since step n - lag you
     *  moved by dp and turned by dq" corrects the CURRENT state -- the update on the pair (present, clone of that step), the
     *  clone recovered from the history ring.  Pose filters only; the window is updateDelayedDev's; commit = false is read-only.
     *  Stream-ordered. */
    void integrateRelativeMeasurementDev(const ukfb_relative_in& in, bool commit = true, const ukfb_relative_out* out = NULL)
    {
        check(ukfb_update_relative_dev(engine, &in, commit ? 1 : 0, out));
    }
    /** host arrays in window order, as updateDelayed: lag / model_per_filter [N] or NULL (lag_uniform / model, a
     *  ukfb_relative_model); z [N][7] (dp, then dq as x y z w), Q [N][6][6] in the tangent order (dp, dtheta); mu_out [N][S] /
     *  cov_out [N][D][D] or NULL: the corrected present state.  Returns the status. */
    std::vector<uint32_t> integrateRelativeMeasurement(int steps, const double* dt, const double* mu_hist, const double* cov_hist,
                                                       int lag_uniform, int model, const double* z, const double* Q, bool commit = true,
                                                       const int32_t* lag = NULL, const int32_t* model_per_filter = NULL,
                                                       const double* in_a = NULL, const double* in_b = NULL, double* mu_out = NULL,
                                                       double* cov_out = NULL, double* maha = NULL, double* loglik = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_relative(engine, steps, dt, mu_hist, cov_hist, in_a, in_b, lag_uniform, lag, model, model_per_filter, z, Q,
                                   commit ? 1 : 0, NULL, NULL, NULL, maha, loglik, st.data(), mu_out, cov_out));
        return st;
    }
    /** Late SENSOR-FRAME samples (ukf_batch_delayed_sensor.h): a lever-arm fix, range or landmark sighting (ukfb_sensor_model)
     *  taken in.lag steps ago corrects the CURRENT state through the history ring -- updateDelayedDev with the h of
     *  updateSensorDev, evaluated on the smoothed state of the sample's own step.  The window is updateDelayedDev's; model 5
     *  reads in.rate_dev, else the rotation-rate ring at the sample's step, else the latch; commit = false is read-only.
     *  Stream-ordered. */
    void updateDelayedSensorDev(const ukfb_delayed_sensor_in& in, bool commit = true, const ukfb_delayed_out* out = NULL)
    {
        check(ukfb_update_delayed_sensor_dev(engine, &in, commit ? 1 : 0, out));
    }
    /** host arrays in window order, as updateDelayed: lag / model_per_filter [N] or NULL (lag_uniform / model, a
     *  ukfb_sensor_model); z [N][3], Q [N][3][3]; mount [N][7] or NULL, then mount_uniform [7] (NULL: r = 0, qs the identity);
     *  point [N][3] or NULL, then point_uniform [3] (NULL: 0); rate [N][3] or NULL; mu_out [N][S] / cov_out [N][D][D] or NULL:
     *  the corrected present state.  Returns the status. */
    std::vector<uint32_t> updateDelayedSensor(int steps, const double* dt, const double* mu_hist, const double* cov_hist, int lag_uniform,
                                              int model, const double* z, const double* Q, const double* mount_uniform = NULL,
                                              const double* point_uniform = NULL, bool commit = true, const int32_t* lag = NULL,
                                              const int32_t* model_per_filter = NULL, const double* mount = NULL,
                                              const double* point = NULL, const double* rate = NULL, const double* in_a = NULL,
                                              const double* in_b = NULL, double* mu_out = NULL, double* cov_out = NULL,
                                              double* maha = NULL, double* loglik = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_update_delayed_sensor(engine, steps, dt, mu_hist, cov_hist, in_a, in_b, lag_uniform, lag, model, model_per_filter, z, Q,
                                         mount, mount_uniform, point, point_uniform, rate, commit ? 1 : 0, NULL, NULL, NULL, maha, loglik,
                                         st.data(), mu_out, cov_out));
        return st;
    }
    /** host arrays in window order, smoothed in place: mu [steps][N][S], cov [steps][N][D][D]; returns the per-filter status */
    std::vector<uint32_t> smooth(int steps, const double* dt, double* mu, double* cov, const double* in_a = NULL,
                                 const double* in_b = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_smooth(engine, steps, dt, mu, cov, in_a, in_b, st.data()));
        return st;
    }
    /** Forecast (ukf_batch.h, "forecast"): `steps` predictions chained from the start record (start_mu [N][S], start_cov
     *  [N][D][D]; both NULL: the filters' current state) WITHOUT committing them.  Exactly one of dt [steps] (every filter's
     *  time step) and ts_us [steps] (stamps, measured against every filter's own last measurement time) is non-NULL; in_a /
     *  in_b [steps][N][3] or NULL (the latched inputs, held over the horizon).  mu [steps][N][S] and cov [steps][N][D][D] (may
     *  be NULL) receive the state after 1 ... steps predictions; steps <= UKFB_FORECAST_MAX_STEPS.  Returns the status. */
    std::vector<uint32_t> forecast(int steps, const double* dt, const int64_t* ts_us, double* mu, double* cov = NULL,
                                   const double* start_mu = NULL, const double* start_cov = NULL, const double* in_a = NULL,
                                   const double* in_b = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap));
        check(ukfb_forecast(engine, steps, dt, ts_us, start_mu, start_cov, in_a, in_b, mu, cov, st.data()));
        return st;
    }
    /** Filter lifecycle (ukf_batch.h, "filter lifecycle"), host forms.  gatherFilters: record k <- filter index[k] (index NULL:
     *  item k is filter k); mu [n][S], cov [n][D][D], last_ts_us [n], initialised [n], each may be NULL; an index outside
     *  [0, capacity()) gives a record of zeros.  Read-only on the engine. */
    void gatherFilters(int64_t n, const int32_t* index, double* mu, double* cov = NULL, int64_t* last_ts_us = NULL,
                       uint8_t* initialised = NULL)
    {
        check(ukfb_gather_filters(engine, n, index, mu, cov, last_ts_us, initialised));
    }
    /** initializeFilter from records: filter index[k] <- (mu[k], cov[k], last_ts_us[k] or 0, initialised[k] or 1; a 0 retires the
     *  filter).  Among the items that name one filter the lowest wins; returns the per-item status (UKFB_ST_INACTIVE: a loser,
     *  or an index outside [0, capacity())). */
    std::vector<uint32_t> scatterFilters(int64_t n, const int32_t* index, const double* mu, const double* cov,
                                         const int64_t* last_ts_us = NULL, const uint8_t* initialised = NULL)
    {
        std::vector<uint32_t> st(static_cast<size_t>(n));
        check(ukfb_scatter_filters(engine, n, index, mu, cov, last_ts_us, initialised, st.data()));
        return st;
    }
    /** clears the initialised flag and the last measurement time of every filter with a non-zero byte in mask_dev [capacity()], a
     *  DEVICE array; stream-ordered */
    void retire(const uint8_t* mask_dev) { check(ukfb_retire_dev(engine, mask_dev)); }
    /** moves the live groups of `group` consecutive filters to the front, in place; new_index / old_index [capacity()] (may be NULL)
     *  receive the maps; returns the number of filters in live groups: the free slots start there.  Bound input buffers are not
     *  moved: permute them with old_index. */
    int64_t compact(int group = 1, int32_t* new_index = NULL, int32_t* old_index = NULL)
    {
        int64_t live = 0;
        check(ukfb_compact(engine, group, new_index, old_index, &live));
        return live;
    }
    std::vector<uint32_t> status()
    {
        std::vector<uint32_t> st(static_cast<size_t>(cap), 0u);
        check(ukfb_get_status(engine, 0, cap, st.data()));
        return st;
    }
    void sync() { check(ukfb_sync(engine)); }

protected:
    void check(int rc) const { if (rc != UKFB_OK) throw std::runtime_error(std::string("pose_estimation engine: ") + ukfb_last_error()); }
    ukfb_engine* engine;
    int64_t cap;
    int S, D, PK;

private:
    BatchUKF(const BatchUKF&);
    BatchUKF& operator=(const BatchUKF&);
};

class BatchPoseUKF : public BatchUKF
{
public:
    BatchPoseUKF(int64_t capacity, int precision = UKFB_F64, int device = 0) : BatchUKF(UKFB_MODEL_POSE, precision, capacity, device)
    {
        double R[144] = {0};   // PoseUKF.cpp:103-107
        for (int k = 0; k < 3; ++k) { R[k * 13] = 0.01; R[(3 + k) * 13] = 0.001; R[(6 + k) * 13] = 0.00001; R[(9 + k) * 13] = 0.00001; }
        setProcessNoiseCovariance(R);
    }
    /** integrateMeasurement(AccelerationMeasurement) per filter; NaN row = none (PoseUKF.cpp:109,175-178) */
    void setAccelerations(int64_t first, int64_t count, const double* acc_mu, const double* acc_cov3x3) { check(ukfb_pose_set_acceleration(engine, first, count, acc_mu, acc_cov3x3)); }
    /** base::samples::RigidBodyState records [N][49] (the layout of ukfb_pose_export_body_states) integrated as measurements of
     *  the blocks `block_mask` selects: the fields as they are, the four 3 x 3 covariances on the diagonal; active [N] or NULL */
    void integrateBodyStates(uint32_t block_mask, const double* records, const uint8_t* active = NULL) { check(ukfb_pose_update_body_states(engine, block_mask, records, active)); }
};

class BatchOrientationUKF : public BatchUKF
{
public:
    BatchOrientationUKF(int64_t capacity, double gyro_bias_tau, double acc_bias_tau, const double earth_rotation[3], int precision = UKFB_F64, int device = 0)
        : BatchUKF(UKFB_MODEL_ORIENT, precision, capacity, device)
    {
        check(ukfb_orient_set_params(engine, gyro_bias_tau, acc_bias_tau, earth_rotation));
    }
    /** initializeFilter plus the reference constructor's input latches (OrientationUKF.cpp:49-50):
     *  rotation_rate.mu = 0 and acceleration.mu = (0, 0, initial gravity), so that a prediction before the first
     *  IMU sample holds the velocity steady exactly as the scalar class does. */
    virtual void initializeFilters(int64_t first, int64_t count, const double* mu, const double* cov)
    {
        BatchUKF::initializeFilters(first, count, mu, cov);
        std::vector<double> gyro(static_cast<size_t>(count) * 3, 0.0), acc(static_cast<size_t>(count) * 3, 0.0);
        for (int64_t i = 0; i < count; ++i) acc[static_cast<size_t>(i) * 3 + 2] = mu[static_cast<size_t>(i) * 14 + 13];
        setInputs(first, count, gyro.data(), acc.data());
    }
    void setInputs(int64_t first, int64_t count, const double* gyro, const double* acc) { check(ukfb_orient_set_inputs(engine, first, count, gyro, acc)); }
    void getRotationRates(int64_t first, int64_t count, double* out) { check(ukfb_orient_get_rotation_rate(engine, first, count, out)); }
};

/** One host process, several MI355X: `total` independent filters in contiguous shards, one engine per device
 *  (ukfb_group_* of ukf_batch.h).  Filters never read each other (UnscentedKalmanFilter.hpp:150), so the shards need no
 *  collective on the data path; gatherMeans is the one exchange (RCCL all-gather over xGMI).  Whole-batch host arrays are
 *  in batch numbering; device-pointer arguments are one pointer PER SHARD (memory on that shard's device). */
class ShardedBatchUKF
{
public:
    virtual ~ShardedBatchUKF() { ukfb_group_destroy(group); }

    int64_t capacity() const { return n; }
    int shards() const { return ukfb_group_size(group); }
    ukfb_group* handle() { return group; }
    /** engine of one shard (every single-engine call of ukf_batch.h applies), its device and filter range */
    ukfb_engine* shard(int r, int* device = NULL, int64_t* first = NULL, int64_t* count = NULL)
    {
        ukfb_engine* e = NULL;
        check(ukfb_group_shard(group, r, &e, device, first, count));
        return e;
    }
    virtual void initializeFilters(int64_t first, int64_t count, const double* mu, const double* cov) { check(ukfb_group_initialize(group, first, count, mu, cov)); }
    void getCurrentStates(int64_t first, int64_t count, double* mu, double* cov, uint8_t* initialised = NULL) { check(ukfb_group_get_state(group, first, count, mu, cov, initialised)); }
    void setProcessNoiseCovariance(const double* R) { check(ukfb_group_set_process_noise(group, R)); }
    void predictionStep(double delta_t) { check(ukfb_group_predict(group, delta_t)); }
    void integrateMeasurements(int model, const double* z, const double* Q) { check(ukfb_group_update(group, model, z, Q)); }
    void cycle(double delta_t, int model, const double* z, const double* Q) { check(ukfb_group_cycle(group, delta_t, model, z, Q)); }
    /** samples already resident on the devices: z_dev[r] / Q_dev[r] on shard r's device, engine precision */
    void cycleDev(double delta_t, int model, const void* const* z_dev, const void* const* Q_dev) { check(ukfb_group_cycle_dev(group, delta_t, model, z_dev, Q_dev)); }
    /** per-filter model ids resident on the devices: meas_model_dev[r] = int32 [filters of shard r] */
    void cycleMixedDev(double delta_t, const int32_t* const* meas_model_dev, const void* const* z_dev, const void* const* Q_dev)
    {
        check(ukfb_group_cycle_mixed_dev(group, delta_t, meas_model_dev, z_dev, Q_dev));
    }
    /** fused predictionStepFromSampleTime(ts[i]) + integrateMeasurement(model[i]) per filter, host arrays over the whole batch */
    void cycleFromSampleTimes(const int64_t* ts_us, const int32_t* model, const double* z, const double* Q) { check(ukfb_group_cycle_timestamps(group, ts_us, model, z, Q)); }
    /** time-ordered asynchronous stream over the sharded batch (filter indices in batch numbering); returns the launches of the shard that needed most */
    int64_t processEvents(int64_t n_events, const int64_t* filter, const int64_t* ts_us, const int32_t* model, const double* z, const double* Q)
    {
        int64_t rounds = 0;
        check(ukfb_group_process_events(group, n_events, filter, ts_us, model, z, Q, NULL, &rounds));
        return rounds;
    }
    /** RCCL all-gather: out_dev[r] ([total][S], engine precision, on shard r's device) receives every filter's mean */
    void gatherMeans(void* const* out_dev) { check(ukfb_group_gather_means(group, out_dev)); }
    uint32_t statusSummary() { uint32_t v = 0; check(ukfb_group_get_status_summary(group, &v)); return v; }
    void sync() { check(ukfb_group_sync(group)); }

protected:
    ShardedBatchUKF(int model, int64_t total, const std::vector<int>& devices, int precision) : group(NULL), n(total)
    {
        if (ukfb_group_create(&group, model, precision, total, devices.data(), static_cast<int>(devices.size())) != UKFB_OK)
            throw std::runtime_error(std::string("pose_estimation: MI355X engine group unavailable: ") + ukfb_last_error());
    }
    void check(int rc) const { if (rc != UKFB_OK) throw std::runtime_error(std::string("pose_estimation engine group: ") + ukfb_last_error()); }
    ukfb_group* group;
    int64_t n;

private:
    ShardedBatchUKF(const ShardedBatchUKF&);
    ShardedBatchUKF& operator=(const ShardedBatchUKF&);
};

class ShardedBatchPoseUKF : public ShardedBatchUKF
{
public:
    ShardedBatchPoseUKF(int64_t total, const std::vector<int>& devices, int precision = UKFB_F64) : ShardedBatchUKF(UKFB_MODEL_POSE, total, devices, precision)
    {
        double R[144] = {0};   // PoseUKF.cpp:103-107
        for (int k = 0; k < 3; ++k) { R[k * 13] = 0.01; R[(3 + k) * 13] = 0.001; R[(6 + k) * 13] = 0.00001; R[(9 + k) * 13] = 0.00001; }
        setProcessNoiseCovariance(R);
    }
    void setAccelerations(int64_t first, int64_t count, const double* acc_mu, const double* acc_cov3x3) { check(ukfb_group_pose_set_acceleration(group, first, count, acc_mu, acc_cov3x3)); }
    void bindAccelerationsDev(const void* const* acc_mu_dev) { check(ukfb_group_pose_bind_acceleration_dev(group, acc_mu_dev)); }
};

class ShardedBatchOrientationUKF : public ShardedBatchUKF
{
public:
    ShardedBatchOrientationUKF(int64_t total, const std::vector<int>& devices, double gyro_bias_tau, double acc_bias_tau, const double earth_rotation[3],
                               int precision = UKFB_F64)
        : ShardedBatchUKF(UKFB_MODEL_ORIENT, total, devices, precision)
    {
        check(ukfb_group_orient_set_params(group, gyro_bias_tau, acc_bias_tau, earth_rotation));
    }
    /** initializeFilter plus the reference constructor's input latches (OrientationUKF.cpp:49-50), as BatchOrientationUKF */
    virtual void initializeFilters(int64_t first, int64_t count, const double* mu, const double* cov)
    {
        ShardedBatchUKF::initializeFilters(first, count, mu, cov);
        std::vector<double> gyro(static_cast<size_t>(count) * 3, 0.0), acc(static_cast<size_t>(count) * 3, 0.0);
        for (int64_t i = 0; i < count; ++i) acc[static_cast<size_t>(i) * 3 + 2] = mu[static_cast<size_t>(i) * 14 + 13];
        setInputs(first, count, gyro.data(), acc.data());
    }
    void setInputs(int64_t first, int64_t count, const double* gyro, const double* acc) { check(ukfb_group_orient_set_inputs(group, first, count, gyro, acc)); }
    void bindInputsDev(const void* const* gyro_dev, const void* const* acc_dev) { check(ukfb_group_orient_bind_inputs_dev(group, gyro_dev, acc_dev)); }
};

}

#endif
