/* ukf_batch.h -- C-ABI of the MI355X-native batched UKF engine (libukf_batch.so).
 *
 * Drop-in boundary for the ONE hot path of rock-slam/slam-pose_estimation: everything the
 * reference reaches through its protected member
 *     boost::shared_ptr<ukfom::ukf<WState> > ukf;          (src/UnscentedKalmanFilter.hpp:150)
 * i.e. ukf->predict / ukf->update / ukf->mu() / ukf->sigma(), plus the per-filter plumbing around
 * it (time gate, latched inputs, process-noise shaping), for a BATCH of independent filters that
 * lives in the HBM of one MI355X.  Host C++ (include/pose_estimation/...hpp) and Python
 * (slam-pose_estimation_amd/engine.py, ctypes) sit on top of exactly these entry points.
 *
 * Conventions
 *  - plain C, opaque handle, int return codes (UKFB_OK == 0); no exception crosses the ABI.
 *  - the caller owns host buffers, the engine owns device buffers.
 *  - calls on one engine must come from one host thread at a time (the reference classes are
 *    boost::noncopyable and single-threaded, UnscentedKalmanFilter.hpp:16).
 *  - every call works on its engine's device and leaves the calling thread's current HIP device as it
 *    found it (one thread may drive engines on several devices, or share the thread with other HIP code).
 *  - work is enqueued on the engine's HIP stream; ukfb_sync() waits for it.  Functions that
 *    copy to host buffers synchronise themselves.
 *  - host-side numeric arrays are double and AoS ("host layout"):
 *      Pose   (UKFB_MODEL_POSE,   S=13, D=12): mu = position(3) orientation(x,y,z,w) velocity(3)
 *              angular_velocity(3)                              (PoseWithVelocity.hpp:18-23)
 *      Orient (UKFB_MODEL_ORIENT, S=14, D=13): mu = orientation(x,y,z,w) velocity(3) bias_gyro(3)
 *              bias_acc(3) gravity(1)                            (OrientationState.hpp:20-26)
 *      cov = D x D row-major (symmetric; the engine stores the lower triangle).
 *    Quaternion order (x,y,z,w) is Eigen's coefficient order.
 *  - "_dev" entry points take DEVICE pointers in the engine's compute precision (float or
 *    double) so that a caller whose inputs are already resident in HBM pays no PCIe copy.
 *    They are consumed on the engine's stream: buffers produced on another stream must be
 *    complete before the call (synchronise, or create the engine on the producer's stream with
 *    ukfb_create_on_stream), and must stay valid AND UNCHANGED until ukfb_sync() or a later
 *    synchronising call returns -- an engine that owns its stream may run a launch as two halves
 *    on two internal streams (ukfb_config.split_streams), so "the next call on the engine" is not
 *    a point after which an input buffer may be rewritten; ukfb_sync() is.
 *  - filters are independent (the reference's are separate objects): no filter's result depends on another filter's
 *    state or inputs.  Reproducibility: the same filter with the same inputs gives the same bits in any launch that
 *    places it in a wavefront whose other three filters run the same number of mean iterations (always the case for the
 *    same batch; also across batch sizes, shards and split launches in every workload of tests/ and bench.py);
 *    otherwise the results agree to the remainder of the re-based rotation deltas, below 4e-14 -- the iteration count
 *    is a wavefront's, a converged filter rides along unchanged.  Filters that commit nothing (uninitialised, gated
 *    out, not factorisable) never influence their wave-mates.
 *  - per-filter failures never abort a call: they are reported in the per-filter status word
 *    (UKFB_ST_*), and a failing filter keeps the state it had before the call (the reference
 *    throws before mutating: UnscentedKalmanFilter.hpp:110-124).
 */
#ifndef UKF_BATCH_H
#define UKF_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ukfb_engine ukfb_engine;

/* ---- return codes ---------------------------------------------------------------------- */
enum {
    UKFB_OK = 0,
    UKFB_ERR_INVALID_ARG = 1,
    UKFB_ERR_NO_DEVICE = 2,   /* no HIP device / HIP runtime error at creation               */
    UKFB_ERR_HIP = 3,         /* HIP runtime error; text via ukfb_last_error()               */
    UKFB_ERR_OUT_OF_RANGE = 4,
    UKFB_ERR_WRONG_MODEL = 5  /* e.g. Orient-only call on a Pose engine                      */
};

/* ---- models / precision ----------------------------------------------------------------- */
enum { UKFB_MODEL_POSE = 0, UKFB_MODEL_ORIENT = 1 };
enum { UKFB_F64 = 0, UKFB_F32 = 1 };

/* measurement model ids = the integrateMeasurement overload they replace */
enum {
    UKFB_MEAS_NONE = -1,            /* filter takes no measurement in this call              */
    UKFB_MEAS_POS3 = 0,             /* PoseUKF.cpp:112-117  PositionMeasurement              */
    UKFB_MEAS_POS_XY = 1,           /* PoseUKF.cpp:119-124  XYMeasurement                    */
    UKFB_MEAS_POS_Z = 2,            /* PoseUKF.cpp:126-131  ZMeasurement                     */
    UKFB_MEAS_ORIENT_SO3 = 3,       /* PoseUKF.cpp:133-138  OrientationMeasurement (axis-angle in) */
    UKFB_MEAS_VEL3 = 4,             /* PoseUKF.cpp:140-145  VelocityMeasurement              */
    UKFB_MEAS_VEL_XY = 5,           /* PoseUKF.cpp:147-152  XYVelocityMeasurement            */
    UKFB_MEAS_VEL_Z = 6,            /* PoseUKF.cpp:154-159  ZVelocityMeasurement             */
    UKFB_MEAS_XVEL_YAWVEL = 7,      /* PoseUKF.cpp:161-166  XVelYawVelMeasurement            */
    UKFB_MEAS_ANGVEL3 = 8,          /* PoseUKF.cpp:168-173  AngularVelocityMeasurement       */
    UKFB_MEAS_ORIENT_BODYVEL3 = 9   /* OrientationUKF.cpp:65-72 VelocityMeasurement (Orient)  */
};

/* ---- per-filter status bits (uint32) ---------------------------------------------------- */
enum {
    UKFB_ST_OK = 0u,
    UKFB_ST_SKIPPED_FIRST_TS = 1u << 0,   /* UnscentedKalmanFilter.hpp:86-90                 */
    UKFB_ST_SKIPPED_SMALL_DT = 1u << 1,   /* UnscentedKalmanFilter.hpp:114-118               */
    UKFB_ST_ERR_NEG_DT = 1u << 2,         /* UnscentedKalmanFilter.hpp:110-113 (throws there) */
    UKFB_ST_ERR_DT_TOO_LARGE = 1u << 3,   /* UnscentedKalmanFilter.hpp:119-122 (throws there) */
    UKFB_ST_ERR_NONFINITE_MEAS = 1u << 4, /* UnscentedKalmanFilter.hpp:142-147 (throws there) */
    UKFB_ST_ERR_CHOLESKY = 1u << 5,       /* ukfom: Cholesky decomposition failed            */
    UKFB_ST_WARN_MEAN_NOCONV = 1u << 6,   /* ukfom: meanSigmaPoints() did not converge       */
    UKFB_ST_UNINITIALISED = 1u << 7,      /* UnscentedKalmanFilter.hpp:53,59                 */
    UKFB_ST_INACTIVE = 1u << 8,           /* filter masked out of this call                  */
    UKFB_ST_REJECTED_GATE = 1u << 9,      /* mahalanobis gate rejected the update            */
    UKFB_ST_ERR_WEIGHTS = 1u << 10,       /* filter banks: the weights of a track are not a distribution */
    UKFB_ST_REPAIRED = 1u << 11           /* covariance conditioning: the covariance or the quaternion was repaired */
};

/* ---- configuration ---------------------------------------------------------------------- */
typedef struct ukfb_config {
    double mean_tol;        /* ukfom meanSigmaPoints tolerance (1e-6)                        */
    int32_t mean_max_iter;  /* ukfom meanSigmaPoints cap (10000, as ukfom)                   */
    double gate_chi2;       /* < 0: accept_any_mahalanobis_distance (PoseUKF.cpp:116)        */
    double min_time_delta;  /* UnscentedKalmanFilter.hpp:31  (1e-9)                          */
    double max_time_delta;  /* UnscentedKalmanFilter.hpp:32  (DBL_MAX)                       */
    int32_t lanes_per_filter; /* 0 / 16 = the tuned layout (one DPP row per filter).  32 / 64 = one or two
                               * filters per wavefront, the brief's literal decomposition kept as an ablation:
                               * fp32 engines only in the shipped library (the fp64 instantiations need AGPRs and
                               * are a diagnostic build option, `make GENERIC_F64=1`); ukfb_layout_supported tells */
    int32_t bucket_models;  /* ukfb_cycle_dev with per-filter model ids (BASELINE config 5's mixed stream): 1 (default) = the
                             * filters are first grouped on the device by what their update costs -- no sample / a linear
                             * sub-state selection (PoseUKF.cpp:7-26,35-69) / the sigma-point path of
                             * OrientationMeasurement (PoseUKF.cpp:28-33,133-138) -- so that every wavefront runs ONE of
                             * the three paths; results are those of 0 (one launch in filter order) to rounding: a filter
                             * never reads another filter's data.  Batches below 16 384 filters are never bucketed.   */
    int32_t split_streams;  /* 1 (default): an engine that owns its stream (ukfb_create with stream = NULL) runs a launch over
                             * 16 384 ... 262 143 filters as two halves on two internal streams, so that the tail of one
                             * launch overlaps the head of the next (small launches lose 4-8 % to their partly empty last
                             * round of workgroups otherwise).  Bit-identical results; every other call joins the two streams
                             * first.  Engines on a caller's stream never split: plain stream order holds for them.        */
    int32_t wide_arithmetic; /* fp32 engines, tuned layout only; 0 (default) = fp32 arithmetic.  1 = the state, the inputs and the
                             * noise tables keep their fp32 format in HBM (same footprint, same C-ABI arrays), but every
                             * instruction of predict / update runs in fp64: values widen on load and narrow on commit.  The
                             * reference computes in fp64 throughout (Measurement.hpp:9-10); an fp32 evaluation of its recursion
                             * leaves the fp64 one by more than 1e-4 after 150 (OrientationState) / 500 (PoseWithVelocity)
                             * cycles of the bench workloads, and no cheaper mix of precisions holds it (DESIGN.md section 3,
                             * profiles/r04_f32_mixed_ab.txt).  This mode does, at the fp64 engine's rate.  Ignored by fp64
                             * engines; ukfb_set_config refuses it together with lanes_per_filter 32 / 64.                     */
    int32_t full_update_check; /* 0 (default): in a FUSED cycle without per-filter timestamps / time steps / activity masks / gate (the streams-only and plain kernels) the update
                             * factorises only the columns of the downdated covariance that applyDelta reads (RT + 3 of them) when
                             * positive definiteness of that covariance is already established: the filter's prediction was committed
                             * in the same launch (its input covariance factorised, the predicted one is a Gram matrix + noise), the
                             * batch-uniform process noise is positive semidefinite with its rotated blocks [0:3] and [3:6] coupled to
                             * no other entry, so that the prediction's rotation keeps it so (checked on the host when it is set) and the
                             * sample's measurement covariance is positive definite (checked per filter in the kernel).  Results are
                             * bit-identical with the complete factorisation; what differs: a covariance that is indefinite through
                             * ROUNDING alone is reported by the next prediction's factorisation (UKFB_ST_ERR_CHOLESKY there), not by
                             * this update.  Any wavefront with a filter that does not meet the conditions, every update-only launch
                             * and every other kernel factorise completely, as ukfom's applyDelta does.  1: always complete.    */
} ukfb_config;

int ukfb_default_config(ukfb_config* cfg);
/* 1 if this build of the library can run `lanes_per_filter` lanes per filter at `precision`, else 0 */
int ukfb_layout_supported(int precision, int lanes_per_filter);

/* ---- lifetime ---------------------------------------------------------------------------- */
/* Replaces `new MTK_UKF(initial_state, state_cov)` per filter (UnscentedKalmanFilter.hpp:42)
 * by one engine holding `capacity` filters on HIP device `device`.  `stream` is a hipStream_t
 * (NULL: the engine creates its own non-blocking stream). */
int ukfb_create(ukfb_engine** out, int model, int precision, int64_t capacity, int device, void* stream);
/* The same, but `stream` is used exactly as given: NULL means the device's DEFAULT stream (hipStreamLegacy semantics),
 * not "create one".  For callers whose buffers are produced on that stream (e.g. a framework's current stream):
 * the "_dev" entry points then need no synchronisation between the producer and the engine. */
int ukfb_create_on_stream(ukfb_engine** out, int model, int precision, int64_t capacity, int device, void* stream);
/* Waits (bounded, see ukfb_sync) for the engine's stream, then frees everything.  If the stream never drains the
 * engine is abandoned without freeing device memory and UKFB_ERR_HIP is returned: exit the process. */
int ukfb_destroy(ukfb_engine* e);
const char* ukfb_last_error(void);
int ukfb_set_config(ukfb_engine* e, const ukfb_config* cfg);
int ukfb_get_config(const ukfb_engine* e, ukfb_config* cfg);
/* Waits for the engine's stream by polling, for at most UKFB_WAIT_TIMEOUT_S seconds (environment, default 120).  A
 * wait that gives up returns UKFB_ERR_HIP ("timed out ...") and POISONS the engine: work of unknown state is still
 * queued, every later call on it fails fast with UKFB_ERR_HIP, and the process is expected to exit non-zero. */
int ukfb_sync(ukfb_engine* e);

/* introspection: model, precision, capacity, S (stored scalars), D (DOF), packed cov length */
int ukfb_describe(const ukfb_engine* e, int* model, int* precision, int64_t* capacity, int* S, int* D, int* PK);

/* ---- state (UnscentedKalmanFilter.hpp:40-75) -------------------------------------------- */
/* initializeFilter(state, cov) for filters [first, first+count): sets mu, cov, marks the filter
 * initialised and zeroes its last_measurement_time (:40-44). */
int ukfb_initialize(ukfb_engine* e, int64_t first, int64_t count, const double* mu, const double* cov);
/* getCurrentState (:51-75): mu and/or cov may be NULL; initialised (uint8 per filter, may be
 * NULL) is the function's bool return. */
int ukfb_get_state(ukfb_engine* e, int64_t first, int64_t count, double* mu, double* cov, uint8_t* initialised);
/* per-filter status words of the most recent predict / update / cycle call */
int ukfb_get_status(ukfb_engine* e, int64_t first, int64_t count, uint32_t* status);
/* OR of all status words of the most recent call (cheap health check) */
int ukfb_get_status_summary(ukfb_engine* e, uint32_t* or_of_all);

/* get/setLastMeasurementTime (:131-133), int64 microseconds as base::Time */
int ukfb_set_last_measurement_time(ukfb_engine* e, int64_t first, int64_t count, const int64_t* t_us);
int ukfb_get_last_measurement_time(ukfb_engine* e, int64_t first, int64_t count, int64_t* t_us);

/* raw device views (engine precision): mu [capacity][S], packed lower-triangular cov
 * [capacity][PK] (row-major: index r(r+1)/2 + c, c <= r), status [capacity]. */
int ukfb_device_views(ukfb_engine* e, void** mu_dev, void** cov_packed_dev, uint32_t** status_dev);

/* ---- process noise / latched inputs ------------------------------------------------------ */
/* setProcessNoiseCovariance (:130): one D x D matrix for the whole batch ...
 * OrientationState engines: predictionStepImpl replaces the two leading 3x3 blocks N of the noise by R N R^T with the
 * rotation matrix R of the current orientation (OrientationUKF.cpp:81-86).  For a batch-uniform noise whose two blocks are
 * exact multiples of the identity, N = s I (the reference's zero default and every BASELINE configuration), the kernels
 * skip the rotation while every orientation quaternion of the wavefront has | |q|^2 - 1 | <= 1e-9 (fp64 engines) / 1e-4
 * (fp32 engines, where the stored norm drifts by ~1e-6 per hundred cycles): R s I R^T = s R R^T, and for Eigen's
 * un-normalised toRotationMatrix R R^T = I + O(|q|^2 - 1).  Deviation from the always-rotating reference: at most
 * 2 | |q|^2 - 1 | s dt^2 per entry and prediction -- 2e-4 relative to a noise entry that is itself ~1e-8 (config 4), i.e.
 * ~1e-12 absolute against covariance entries of 1e-4 ... 1e-2 whose fp32 rounding is 1e-11 ... 1e-9: below the
 * arithmetic's own rounding (profiles/r03_f32_drift_attribution.txt: the always-rotating build `d_iso` gives the same
 * distances to the oracle).  Anisotropic blocks, per-filter noise and non-unit quaternions take the rotated path. */
int ukfb_set_process_noise(ukfb_engine* e, const double* R);
/* ... or one per filter ([count][D][D]); the first per-filter call switches the engine to
 * per-filter storage (initialised from the batch-uniform matrix). */
int ukfb_set_process_noise_per_filter(ukfb_engine* e, int64_t first, int64_t count, const double* R);
int ukfb_get_process_noise(ukfb_engine* e, int64_t filter, double* R);

/* PoseUKF::integrateMeasurement(AccelerationMeasurement) (PoseUKF.cpp:175-178): latch acc.mu per
 * filter ([count][3]; a NaN row = "no acceleration", the ctor default PoseUKF.cpp:109) and the
 * batch-uniform acc.cov (3x3; NULL keeps the current one, default Identity, Measurement.hpp:12). */
int ukfb_pose_set_acceleration(ukfb_engine* e, int64_t first, int64_t count, const double* acc_mu,
                               const double* acc_cov);
/* device-resident variant: acc_mu_dev [capacity][3] in engine precision, used directly (no copy)
 * by later predict/cycle calls until replaced; NULL returns to the engine-owned buffer. */
int ukfb_pose_bind_acceleration_dev(ukfb_engine* e, const void* acc_mu_dev);

/* OrientationUKF ctor parameters (OrientationUKF.cpp:41-51): taus and earth rotation vector. */
int ukfb_orient_set_params(ukfb_engine* e, double gyro_bias_tau, double acc_bias_tau, const double earth_rotation[3]);
/* OrientationUKF::integrateMeasurement(RotationRate / Acceleration) (:53-63): latch per filter;
 * either pointer may be NULL to leave that input unchanged.  Non-finite rows are rejected
 * per filter (status ERR_NONFINITE_MEAS, previous value kept) as checkMeasurment does (:55,61). */
int ukfb_orient_set_inputs(ukfb_engine* e, int64_t first, int64_t count, const double* gyro, const double* acc);
int ukfb_orient_bind_inputs_dev(ukfb_engine* e, const void* gyro_dev, const void* acc_dev);
/* OrientationUKF::getRotationRate (:74-77) for filters [first, first+count): out [count][3] */
int ukfb_orient_get_rotation_rate(ukfb_engine* e, int64_t first, int64_t count, double* out);

/* ---- BodyStateMeasurement adapters (pose_with_velocity/BodyStateMeasurement.hpp:14-39) ---- */
/* One record per filter, 49 doubles: position(3) orientation(x,y,z,w) velocity(3) angular_velocity(3)
 * cov_position(9) cov_orientation(9) cov_velocity(9) cov_angular_velocity(9) (3x3 blocks, row-major) --
 * the fields of base::samples::RigidBodyState that the reference converts.
 * export = toRigidBodyState (:28-39): velocity is rotated into the navigation frame,
 *          velocity_out = orientation * velocity (:32); the blocks are the diagonal 3x3 blocks (:35-38).
 * import = fromRigidBodyState (:14-26) followed by initializeFilter: fields copied as they are (no inverse
 *          rotation, as in the reference), covariance = the four blocks at (0,0) (3,3) (6,6) (9,9), zero
 *          elsewhere (:21-25).  Pose engines only. */
#define UKFB_BODY_STATE_SCALARS 49
int ukfb_pose_export_body_states(ukfb_engine* e, int64_t first, int64_t count, double* out);
int ukfb_pose_import_body_states(ukfb_engine* e, int64_t first, int64_t count, const double* in);

/* ---- predict (UnscentedKalmanFilter.hpp:83-125 + predictionStepImpl) --------------------- */
/* predictionStep(delta_t) with one dt for every filter */
int ukfb_predict(ukfb_engine* e, double dt);
/* predictionStep(delta_t[i]) (host array [capacity]) */
int ukfb_predict_dt(ukfb_engine* e, const double* dt);
/* predictionStepFromSampleTime(ts[i]) (host array [capacity], int64 microseconds) */
int ukfb_predict_timestamps(ukfb_engine* e, const int64_t* ts_us);
/* device-resident variants (double / int64 device arrays [capacity]) */
int ukfb_predict_dt_dev(ukfb_engine* e, const double* dt_dev);
int ukfb_predict_timestamps_dev(ukfb_engine* e, const int64_t* ts_us_dev);

/* ---- update (integrateMeasurement -> ukf->update) ---------------------------------------- */
/* One model id for the batch.  z [capacity][3] (first m entries used; axis-angle for ORIENT_SO3),
 * Q [capacity][3][3] (leading m x m block used), active (uint8 [capacity], may be NULL = all). */
int ukfb_update(ukfb_engine* e, int meas_model, const double* z, const double* Q, const uint8_t* active);
/* per-filter model ids (int32 [capacity]; negative = no measurement for that filter) */
int ukfb_update_mixed(ukfb_engine* e, const int32_t* meas_model, const double* z, const double* Q);
/* device-resident variants: z_dev [capacity][3], Q_dev [capacity][9] in engine precision;
 * meas_model_dev int32 [capacity] or NULL (then meas_model_uniform applies to every filter). */
int ukfb_update_dev(ukfb_engine* e, int meas_model_uniform, const int32_t* meas_model_dev, const void* z_dev,
                    const void* Q_dev);

/* ---- fused cycle: predictionStep(dt) followed by integrateMeasurement, one launch -------- */
/* The host-array forms (ukfb_cycle, ukfb_cycle_uniform_q) upload their samples on a separate copy stream into one of two
 * staging sets, so that the upload of call k + 1 overlaps the kernel of call k; they return when the caller's arrays have been
 * consumed (the arrays may be rewritten at once), not when the kernel is done. */
int ukfb_cycle(ukfb_engine* e, double dt, int meas_model, const double* z, const double* Q);
int ukfb_cycle_dev(ukfb_engine* e, double dt, int meas_model_uniform, const int32_t* meas_model_dev, const void* z_dev,
                   const void* Q_dev);

/* One measurement covariance for the whole batch (the usual case: a sensor's covariance is a constant): Q9 is ONE 3x3
 * (9 doubles / 9 engine-precision scalars on the device; leading m x m block used).  Same results as the per-filter
 * forms with that matrix repeated; a quarter of the bytes across PCIe and no per-filter Q stream in the kernel. */
int ukfb_update_uniform_q(ukfb_engine* e, int meas_model, const double* z, const double* Q9, const uint8_t* active);
int ukfb_cycle_uniform_q(ukfb_engine* e, double dt, int meas_model, const double* z, const double* Q9);
int ukfb_cycle_uniform_q_dev(ukfb_engine* e, double dt, int meas_model, const void* z_dev, const void* Q9_dev);

/* `cycles` consecutive fused cycles in ONE launch (replay of buffered samples, catching up after a stall, fixed-rate
 * sensors whose samples are batched): predictionStep(dt) + integrateMeasurement(meas_model) `cycles` times for every
 * filter, exactly as `cycles` calls of ukfb_cycle_dev would -- same arithmetic, bit-identical state -- but the filter
 * stays in LDS between its cycles: the state crosses HBM once per launch instead of once per cycle.
 * The samples sit in rings of `slots` input sets on the device, engine precision: z_dev [slots][capacity][3],
 * Q_dev [slots][capacity][9]; cycle c (0-based) reads slot (first_slot + c) % slots.  in_a_dev / in_b_dev
 * ([slots][capacity][3], either may be NULL) replace the latched inputs per cycle in the same way -- Pose: in_a =
 * acceleration (acc.mu of integrateMeasurement(AccelerationMeasurement), PoseUKF.cpp:175-178; NaN = no acceleration,
 * constant-velocity branch), in_b unused; Orient: in_a = acceleration.mu, in_b = rotation_rate.mu
 * (OrientationUKF.cpp:53-63); NULL: the inputs latched in the engine serve every cycle.  The latches themselves are
 * not modified.  After the call the status word of a filter is the OR over its cycles; a cycle whose prediction is
 * gated or fails is skipped for that filter as in a single launch, the following cycles still run. */
int ukfb_cycle_multi_dev(ukfb_engine* e, int cycles, double dt, int meas_model, int slots, int first_slot,
                         const void* in_a_dev, const void* in_b_dev, const void* z_dev, const void* Q_dev);
/* the same with per-filter model ids per cycle (the asynchronous mixed stream of BASELINE config 5, buffered):
 * meas_model_dev is a ring int32 [slots][capacity] like z and Q, negative = no measurement for that filter in that cycle
 * (prediction only, status INACTIVE as in ukfb_cycle_dev) */
int ukfb_cycle_multi_mixed_dev(ukfb_engine* e, int cycles, double dt, int slots, int first_slot, const void* in_a_dev,
                               const void* in_b_dev, const int32_t* meas_model_dev, const void* z_dev, const void* Q_dev);
/* ukfb_cycle_multi_dev with a schedule: cycle c predicts by dt[c] and updates with model meas_model[c] (host arrays of `cycles`
 * entries; a negative model = prediction only in that cycle, i.e. a plain predictionStep).  One launch per 32 cycles.  This is an IMU-rate filter with slower aiding sensors replayed from a buffer: e.g. ten 100 Hz
 * predictions of which the last one carries a 10 Hz position fix (BASELINE config 2's workload) in one launch. */
int ukfb_cycle_schedule_dev(ukfb_engine* e, int cycles, const double* dt, const int32_t* meas_model, int slots, int first_slot,
                            const void* in_a_dev, const void* in_b_dev, const void* z_dev, const void* Q_dev);
/* ukfb_cycle_multi_dev from host arrays of doubles, one input set per cycle: z [cycles][capacity][3], Q [cycles][capacity][3][3],
 * in_a / in_b [cycles][capacity][3] or NULL (uploaded to an engine-owned ring, then one launch) */
int ukfb_cycle_multi(ukfb_engine* e, int cycles, double dt, int meas_model, const double* in_a, const double* in_b,
                     const double* z, const double* Q);

/* fused predictionStepFromSampleTime(ts[i]) + integrateMeasurement(model[i]) per filter, one launch.
 * ts_us[i] < 0: filter i has no sample in this call (untouched, status INACTIVE);
 * model[i] < 0: prediction only.  Host arrays [capacity] / device arrays in engine precision. */
int ukfb_cycle_timestamps(ukfb_engine* e, const int64_t* ts_us, const int32_t* meas_model, const double* z, const double* Q);
int ukfb_cycle_timestamps_dev(ukfb_engine* e, const int64_t* ts_us_dev, const int32_t* meas_model_dev, const void* z_dev,
                              const void* Q_dev);

/* ---- time-ordered asynchronous measurement stream ------------------------------------------ */
/* What Rock's stream aligner (drivers/aggregator, manifest.xml:14) does for one filter, for a batch:
 * n_events samples (filter index, timestamp, model id, z[3], Q[3][3]) arrive in ANY order.  Per filter
 * they are applied in timestamp order (stable for equal stamps), each as
 * predictionStepFromSampleTime(ts) followed by integrateMeasurement(model) (model < 0: prediction
 * only).  Filters are independent, so the r-th sample of every filter forms round r and each round
 * is one fused launch.  After the call ukfb_get_status returns, per filter, the OR of its status
 * words over all rounds; status_or / rounds (may be NULL) receive the batch-wide OR and the number
 * of launches. */
int ukfb_process_events(ukfb_engine* e, int64_t n_events, const int64_t* filter, const int64_t* ts_us,
                        const int32_t* meas_model, const double* z, const double* Q, uint32_t* status_or, int64_t* rounds);
/* Same stream already resident in HBM (z, Q in the engine's precision): ordering (two stable radix sorts:
 * timestamp, then filter index), ranking and the per-round scatter all run on the device; the host only
 * learns the number of rounds.  The host-pointer variant above uploads the five arrays and calls this. */
int ukfb_process_events_dev(ukfb_engine* e, int64_t n_events, const int64_t* filter_dev, const int64_t* ts_us_dev,
                            const int32_t* meas_model_dev, const void* z_dev, const void* Q_dev, uint32_t* status_or,
                            int64_t* rounds);


/* ---- innovation statistics and measurement association, WITHOUT an update ------------------------------------------------ */
/* The first half of ukf::update -- predicted measurement z-bar, innovation covariance S, innovation nu = z (-) z-bar, squared
 * Mahalanobis distance d^2 = nu^T S^-1 nu (the normalised innovation squared) and the measurement log-likelihood -- for up to
 * 32 CANDIDATE samples per filter, and the candidate nearest to the filter inside the chi-square gate.  ukfom makes the
 * acceptance test a predicate at every call site (accept_any_mahalanobis_distance, PoseUKF.cpp:116); with these numbers a
 * caller evaluates any predicate, associates detections with filters, monitors consistency or weights a bank of filters.
 * The call is READ-ONLY: mean, covariance, last measurement time, latched inputs and the engine's own status array are bit
 * for bit what they were.  It is stream-ordered like every "_dev" call.
 *  - z_dev [candidates][capacity][3] -- the slot layout of ukfb_cycle_multi_dev's sample ring, so a buffered ring is scored
 *    as it lies; Q_dev [capacity][9], or ONE 3x3 when q_is_uniform (as ukfb_update_uniform_q); candidates 1 ... 32; model ids
 *    and the axis-angle input of UKFB_MEAS_ORIENT_SO3 exactly as ukfb_update_dev.
 *  - status (of THIS call): UNINITIALISED; INACTIVE (model id negative or not one of the engine's); ERR_CHOLESKY (the
 *    covariance is not factorisable in the columns the measurement reads, or S is not positive definite -- the sub-state
 *    selections of PoseWithVelocity read S = Sigma[sel][sel] + Q in closed form, as the update kernels do, so for them it is S
 *    that is judged); WARN_MEAN_NOCONV.  A filter with one of the first three writes NaN to its float outputs and -1 to best.
 *    A candidate with a non-finite entry among its first m gets NaN innov / maha / loglik and is never best;
 *    ERR_NONFINITE_MEAS is set when EVERY candidate of the filter is non-finite.
 *  - the arithmetic is the update kernels' (same device functions, same order), so maha[k] is the number ukfb_update_dev
 *    compares with ukfb_config.gate_chi2 for candidate k.  The kernel is the tuned one-row-per-filter layout for every
 *    lanes_per_filter setting; fp32 engines with wide_arithmetic compute in fp64 and store fp32.
 *  - device groups: ukfb_group_shard hands out each shard's engine, on which these per-engine calls work. */
typedef struct ukfb_innovation_out {   /* device pointers, engine precision; any may be NULL */
    void*     z_pred;   /* [capacity][4]  z-bar: first m entries (rest 0); ORIENT_SO3: quaternion x,y,z,w */
    void*     S;        /* [capacity][9]  row-major 3x3, leading m x m block = S, rest 0                    */
    void*     innov;    /* [candidates][capacity][3]  nu = z (-) z-bar, first m entries (rest 0)             */
    void*     maha;     /* [candidates][capacity]     d^2 = nu^T S^-1 nu                                     */
    void*     loglik;   /* [candidates][capacity]     -0.5 (d^2 + ln det S + m ln 2 pi)                      */
    int32_t*  best;     /* [capacity]  candidate with the smallest d^2 among those that are finite and, if
                           cfg.gate_chi2 >= 0, have d^2 <= gate_chi2 (the update's own comparison); -1: none;
                           equal d^2: the lower candidate index                                              */
    uint32_t* status;   /* [capacity]  UKFB_ST_* of THIS call (the engine's own status array is not written) */
} ukfb_innovation_out;

int ukfb_innovation_dev(ukfb_engine* e, int meas_model_uniform, const int32_t* meas_model_dev, int candidates,
                        const void* z_dev, const void* Q_dev, int q_is_uniform, const ukfb_innovation_out* out);
/* z_sel[i] = z[best[i]][i] (zeros where best[i] < 0) and meas_model_sel[i] = best[i] < 0 ? -1 : model(i) (may be NULL), so
 * that ukfb_update_dev(e, 0, meas_model_sel, z_sel, Q) -- or ukfb_cycle_dev -- finishes nearest-neighbour association with
 * no host round trip: filters without an accepted candidate are left untouched (status INACTIVE). */
int ukfb_select_candidates_dev(ukfb_engine* e, int candidates, const int32_t* best_dev, int meas_model_uniform,
                               const int32_t* meas_model_dev, const void* z_dev, void* z_sel_dev, int32_t* meas_model_sel_dev);
/* host arrays of doubles (z [candidates][capacity][3], Q [capacity][3][3]), any output NULL; synchronises */
int ukfb_innovation(ukfb_engine* e, int meas_model, int candidates, const double* z, const double* Q, double* z_pred,
                    double* S, double* innov, double* maha, double* loglik, int32_t* best, uint32_t* status);


/* ---- filter banks: IMM mixing, weights and mixture moments ---------------------------------------------------------------- */
/* An engine of `capacity` filters read as T = capacity / M TRACKS of M = `hypotheses` HYPOTHESES, track-major: hypothesis j of
 * track t is filter t * M + j (e.g. a quiet and a manoeuvring process noise set per filter, or PoseUKF's constant-velocity and
 * acceleration branches through per-filter NaN acceleration rows).  2 <= M <= 8; capacity % M != 0 is UKFB_ERR_INVALID_ARG.
 * All device arrays in engine precision; stream-ordered like every "_dev" call: no host synchronisation, no allocation at
 * call time.  The same kernels serve every lanes_per_filter setting; fp32 engines compute in fp32, with wide_arithmetic in
 * fp64 (stored fp32).  The engine's own status array, last measurement times, latched inputs and noise are never written.
 *
 * MIXTURE MOMENTS of a track under weights w_j >= 0, sum_j w_j = 1 ((+) / (-): the engine's, right multiplication on SO(3)):
 *   1. ref = mu_j*, j* the hypothesis of the largest weight (ties: the lowest index);
 *   2. d = sum_j w_j (mu_j (-) ref), ref <- ref (+) d, ukfom's stopping rule as for the sigma-point means
 *      (do ... while (|d| > mean_tol && ++it < mean_max_iter)); mean = ref; the cap sets UKFB_ST_WARN_MEAN_NOCONV;
 *   3. delta_j = mu_j (-) mean; J_j = the D x D identity with its SO(3) block replaced by
 *      Jr^-1(phi) = I + [phi]x / 2 + c(theta) [phi]x^2, phi = the rotation part of delta_j, theta = |phi|,
 *      c = 1/theta^2 - (1 + cos theta) / (2 theta sin theta): the first-order transport of a covariance from the tangent
 *      space at mu_j to the one at the mean, (mu_j (+) eps) (-) mean = delta_j + J_j eps + O(eps^2);
 *   4. cov = sum_j w_j (J_j Sigma_j J_j^T + delta_j delta_j^T);
 *   5. a hypothesis of weight exactly 0 is skipped (selected out, not multiplied by 0): whatever its state holds, NaN
 *      included, never reaches the result.  One-hot weights return that hypothesis bit for bit.
 * Per-TRACK status, written to the caller's array ([T], may be NULL):
 *   UNINITIALISED     any hypothesis of the track is uninitialised;
 *   ERR_WEIGHTS       a weight is negative or non-finite, or |sum_j w_j - 1| > 16 M eps, eps the machine epsilon of the
 *                     engine's storage precision (2^-52 / 2^-23); the w_out of ukfb_bank_weights_dev meets this bound by
 *                     construction (w_out = e_j / sum e_j with e_j = exp(a_j - max a));
 *   WARN_MEAN_NOCONV  the mean iteration hit its cap (mean_max_iter); the mean is the last iterate.
 * A track with either of the first two writes NaN to its outputs (combine) or is left bit for bit untouched (mix). */

/* logw_out[t][j] = logw_in[t][j] + loglik[t][j] - logsumexp_j(logw_in + loglik), w_out = exp(logw_out) (may be NULL).
 * logw_in = NULL: uniform prior; loglik = NULL: normalise only.  A NaN loglik (what ukfb_innovation_dev writes for a filter it
 * could not score) kills that hypothesis: weight 0, logw_out = -inf.  Every hypothesis of a track dead: ERR_WEIGHTS, and
 * logw_out is logw_in normalised on its own (uniform if that is not a distribution either). */
int ukfb_bank_weights_dev(ukfb_engine* e, int hypotheses, const void* logw_in_dev, const void* loglik_dev,
                          void* logw_out_dev, void* w_out_dev, uint32_t* status_dev);
/* One estimate per track: w_dev [capacity], mu_out_dev [T][S], cov_packed_out_dev [T][PK] (lower triangle as
 * ukfb_device_views; may be NULL).  READ-ONLY on the engine. */
int ukfb_bank_combine_dev(ukfb_engine* e, int hypotheses, const void* w_dev, void* mu_out_dev, void* cov_packed_out_dev,
                          uint32_t* status_dev);
/* IMM interaction: with the row-stochastic `transition` (HOST, [M][M], transition[j][i] = P(model i now | model j before);
 * checked on the host: finite, non-negative, rows sum to 1 within 1e-12; passed to the kernel by value),
 *   c_i = sum_j transition[j][i] w_j,  w_{j|i} = transition[j][i] w_j / c_i,
 * hypothesis i of every track is REPLACED (mean and covariance) by the mixture moments of all M hypotheses -- as they were
 * before the call -- under w_{.|i}, and w_pred_out_dev [capacity] receives c_i.  c_i = 0 exactly: hypothesis i keeps its
 * state, w_pred = 0.  A failing track (above) keeps every bit and gets w_pred = w. */
int ukfb_bank_mix_dev(ukfb_engine* e, int hypotheses, const void* w_dev, const double* transition, void* w_pred_out_dev,
                      uint32_t* status_dev);
/* host arrays of doubles: w [capacity], mu [T][S], cov [T][D][D] (may be NULL), status [T] (may be NULL); synchronise */
int ukfb_bank_combine(ukfb_engine* e, int hypotheses, const double* w, double* mu, double* cov, uint32_t* status);
int ukfb_bank_mix(ukfb_engine* e, int hypotheses, const double* w, const double* transition, double* w_pred, uint32_t* status);

/* ---- fixed-interval smoothing: a manifold Rauch-Tung-Striebel backward pass -------------------------------------------- */
/* The estimate of step k given the WHOLE window (a track's past after an association is confirmed, an offline trajectory,
 * fixed-lag output a few cycles behind real time), without a round trip through the host.
 * A HISTORY is a ring of `slots` copies of the engine's state in the engine's own device format: mu_hist [slots][capacity][S],
 * cov_hist [slots][capacity][PK] (packed lower triangle, as ukfb_device_views), engine precision.  A WINDOW is `steps`
 * consecutive slots, oldest first: step c (0 ... steps - 1) lives in slot (first_slot + c) % slots -- the convention of the
 * sample rings of ukfb_cycle_multi_dev.  Step c holds the FILTERED state at time c (after that time's update, before the
 * prediction to c + 1); dt[c] (HOST, steps - 1 entries, passed to the kernels by value) is the time step of the prediction
 * c -> c + 1.  in_a_dev / in_b_dev: optional input rings [slots][capacity][3] indexed like the history (slot of step c = the
 * inputs of the prediction c -> c + 1), with the meaning they have in ukfb_cycle_multi_dev, the per-filter NaN acceleration row
 * that selects PoseUKF's constant-velocity branch included; NULL: the engine's latched inputs serve every step.  Process noise
 * (batch-uniform or per filter), acc.cov, the taus, the earth rotation, mean_tol, mean_max_iter and min / max_time_delta are
 * the engine's at the time of the call.
 *
 * Per filter ((+) / (-): the engine's, right multiplication on SO(3)): (mu^s, Sigma^s) at step steps - 1 is the filtered state
 * of that step, bit for bit; then for c = steps - 2 ... 0, with (mu, Sigma) the history's step c:
 *   1. the prediction from (mu, Sigma) by dt[c] with step c's inputs is REDONE exactly as ukfb_predict makes it (noise shaping
 *      and the acceleration-branch rule of PoseUKF.cpp:188-193 included): L = chol(Sigma), sigma points X_i, Y_i = g(X_i), the
 *      iterated mean mu^-, delta_i = Y_i (-) mu^-, Sigma^- = 1/2 sum_i delta_i delta_i^T + R;
 *   2. C = 1/2 sum_i (X_i (-) mu) delta_i^T  (D x D, not symmetric; X_j+- (-) mu = +-L col j, which the kernel uses);
 *   3. G = C (Sigma^-)^-1 through a Cholesky factorisation of Sigma^- and two triangular solves per row;
 *   4. e = mu^s_(c+1) (-) mu^-; Sigma^t = J Sigma^s_(c+1) J^T, J the identity but for the SO(3) block Jr^-1(phi), phi the
 *      rotation part of e (the transport of the filter banks above);
 *   5. Sigma~ = Sigma + G (Sigma^t - Sigma^-) G^T (the lower triangle is computed);
 *   6. (mu^s_c, Sigma^s_c) = applyDelta(mu, Sigma~, G e), the update's own commit: Sigma~ is factorised and re-sampled around
 *      mu (+) G e.
 * Status of the call, written to the caller's array ([capacity], may be NULL) as the OR over the steps:
 *   SKIPPED_SMALL_DT / ERR_NEG_DT / ERR_DT_TOO_LARGE  dt[c] is gated (<= min_time_delta, < 0, > max_time_delta): the forward
 *                     pass made no prediction there, step c receives the bits of step c + 1's smoothed state;
 *   ERR_CHOLESKY      Sigma, Sigma^- or Sigma~ of a step is not positive definite: that step's smoothed state is its filtered
 *                     state, bit for bit, and the chain continues from it;
 *   WARN_MEAN_NOCONV  the mean iteration hit its cap (mean_max_iter); the last iterate is used;
 *   UNINITIALISED     nothing is written for that filter.
 * A filter that fails, is gated or is uninitialised never changes the bits of another filter.  The calls are READ-ONLY on the
 * engine: mean, covariance, last measurement times, latches, noise and the engine's own status array keep every bit.
 * Device groups: per shard through ukfb_group_shard. */

/* Stream-ordered copy of the engine's current mean and packed covariance into slot `slot` of the caller's rings.  Needed, not
 * a convenience: an engine that owns its stream may run a launch as two halves on two internal streams (split_streams), so a
 * caller cannot order a copy of ukfb_device_views behind a launch without ukfb_sync; this call joins the streams as every
 * other call does.  No host synchronisation; the first push of an engine creates the one-record workspace that
 * ukfb_smooth_dev needs for windows without a covariance output, no later push allocates. */
int ukfb_history_push_dev(ukfb_engine* e, int slots, int slot, void* mu_hist_dev, void* cov_hist_dev);
/* 2 <= steps <= slots.  mu_out_dev / cov_out_dev: rings of the history's shape and indexing; they may be the history itself
 * (in place), and cov_out_dev may be NULL.  Between the steps of a launch the smoothed state stays in LDS; a launch covers at
 * most 32 backward steps, longer windows are chained by the host and the next launch starts from the smoothed state the
 * previous one stored (with cov_out_dev = NULL the chain's covariance crosses that boundary through the engine's one-record
 * workspace, which ukfb_history_push_dev created; only an engine that never pushed creates it here, once).  Stream-ordered, no
 * host synchronisation, no allocation at call time.  The same
 * kernel serves every lanes_per_filter setting; fp32 engines compute in fp32, with wide_arithmetic in fp64 (stored fp32). */
int ukfb_smooth_dev(ukfb_engine* e, int steps, const double* dt, int slots, int first_slot, const void* mu_hist_dev,
                    const void* cov_hist_dev, const void* in_a_dev, const void* in_b_dev, void* mu_out_dev, void* cov_out_dev,
                    uint32_t* status_dev);
/* host arrays of doubles in window order, smoothed IN PLACE: mu [steps][capacity][S], cov [steps][capacity][D][D];
 * in_a / in_b [steps][capacity][3] or NULL (the latched inputs); status [capacity] (may be NULL); synchronises */
int ukfb_smooth(ukfb_engine* e, int steps, const double* dt, double* mu, double* cov, const double* in_a, const double* in_b,
                uint32_t* status);

/* ---- late samples: a delayed-measurement update through the state history -------------------------------------------------- */
/* A sample that was taken `lag` steps ago (a GPS, USBL or visual fix behind the inertial stream) corrects the CURRENT state,
 * without storing measurements and without replaying cycles: the smoother's backward chain runs from the present down to the
 * step of the sample, the product of its gains is the cross-covariance between that step and the present, and the sample's
 * update of the smoothed past state is carried to the present through it.  For a linear system the result is what the filter
 * would hold had the sample arrived in order; whatever mix of update calls produced the history, the call only needs the ring.
 *
 * WINDOW: ukfb_smooth_dev's -- `steps` consecutive slots of a history ring (mu_hist_dev [slots][capacity][S], cov_hist_dev
 * [slots][capacity][PK], engine precision), oldest first, step c in slot (first_slot + c) % slots holding the filtered state of
 * time c; dt[c] (HOST, steps - 1 entries, by value; may be NULL for steps = 1) the step of the prediction c -> c + 1; in_a_dev /
 * in_b_dev optional input rings with the smoother's meaning, NULL: the engine's latches.  One difference: STEP n = steps - 1 IS
 * THE ENGINE'S OWN CURRENT STATE, read from the engine; the ring's slot of step n is never read (a caller who pushes after every
 * cycle has it there anyway).  1 <= steps <= min(slots, UKFB_DELAYED_MAX_STEPS); more steps is UKFB_ERR_OUT_OF_RANGE and
 * writes nothing.  Keeping the engine's state, process noise and inputs consistent with what the ring recorded is the caller's
 * responsibility.
 * LAG: every filter has a lag l >= 0, its sample was taken at step s = n - l: lag_uniform, or lag_dev [capacity] (int32) when
 * that pointer is non-NULL.  l = 0 is an ordinary update.  A negative lag: no sample for that filter (INACTIVE).  l > steps - 1:
 * the sample is older than the window reaches -- UKFB_ST_ERR_NEG_DT, the status a late sample gets from the cycle calls, and
 * the filter keeps every bit.
 * SAMPLE: the measurement models of ukfb_update_dev, ids 0 ... 9, uniform or per filter (meas_model_dev; a negative id or one
 * the engine's model does not have: INACTIVE); z_dev [capacity][3] (axis-angle for the SO(3) model, as ukfb_update_dev);
 * Q_dev [capacity][9] or one 3 x 3 with q_is_uniform.  State-block models are not served; sensor-frame models: ukf_batch_delayed_sensor.h.
 *
 * Per filter ((+) / (-): the engine's; J(phi): the identity with Jr^-1(phi) on the SO(3) block, the smoother's transport;
 * A(phi): the identity with Jr(phi) = I - (1 - cos t) / t^2 [phi]x + (t - sin t) / t^3 [phi]x^2 there):
 *   1. (mu^s_n, Sigma^s_n) = the engine's (mu_n, Sigma_n), M_n = I (D x D);
 *   2. for c = n - 1 ... s: the smoother's steps 1-6 exactly as ukfb_smooth_dev defines them (the redone prediction, C, G_c,
 *      e = mu^s_(c+1) (-) mu^-_(c+1), the transport J(e_rot), Sigma~, the commit applyDelta(mu_c, Sigma~, delta_c = G_c e)) give
 *      (mu^s_c, Sigma^s_c), and M_c = A(delta_c,rot) G_c J(e_rot) M_(c+1).  J re-expresses a deviation about mu^s_(c+1) as one
 *      about mu^-_(c+1); A re-expresses a deviation about the filtered mu_c as one about mu^s_c = mu_c (+) delta_c, to first
 *      order what applyDelta's re-sampling does to the covariance.  M_s Sigma_n is Cov(x_s about mu^s_s, x_n about mu_n | all
 *      samples up to n).  A gated dt[c] (small, negative, too large) passes chain and M through, as the smoother passes its chain;
 *   3. ukfom's update, first half, on (mu^s_s, Sigma^s_s): L = chol(Sigma^s_s), sigma points, Z_i = h(X_i), the iterated mean
 *      z-bar, S = 1/2 sum dz dz^T + Q, C_z = sum_j (L col j) W_j^T, S = Ls Ls^T, Y_s = C_z Ls^-T, nu = z (-) z-bar,
 *      y = Ls^-1 nu, d^2 = |y|^2, ln det S; the gate is ukfb_update_dev's (gate_chi2);
 *   4. Y_n = Sigma_n M_s^T (Sigma^s_s)^-1 Y_s (two triangular solves with L per row of Sigma_n M_s^T); for l = 0 this is Y_s;
 *   5. Sigma~_n = Sigma_n - Y_n Y_n^T, (mu_n, Sigma_n) <- applyDelta(mu_n, Sigma~_n, Y_n y), the update's own commit.
 * The residual offset of a sample inside its step interval is ignored (ukfb_delayed_lag_dev picks the nearest step).
 * LIMITATION: the ring is not rewritten after a commit.  A second late sample for the same filter inside the same window runs
 * its chain over records that do not know the first: its result is approximate (tests/test_delayed_reference.py records by how
 * much on a linear system).  The last measurement times of the engine are not moved: the sample is older than they are.
 *
 * commit = 0 is READ-ONLY on the engine (as ukfb_innovation_dev): only the outputs are written.  commit = 1 stores the corrected
 * state into the engine; `out` may then be NULL.  Outputs (device, engine precision, any may be NULL): z_pred [capacity][4] (a
 * quaternion for the SO(3) model, else the first m entries and zeros), S [capacity][9] (zeros beyond m), innov [capacity][3],
 * maha, loglik [capacity], status [capacity] (uint32), and mu_out [capacity][S] / cov_out [capacity][PK], the corrected present
 * state: commit = 0 shows there what commit = 1 would store.  mu_out / cov_out must NOT be the engine's own arrays or the ring.
 * Status of the call (with commit = 1 also written to the engine's status array):
 *   UNINITIALISED; INACTIVE (negative lag, no model); ERR_NEG_DT (out of the window); ERR_NONFINITE_MEAS (a used entry of z);
 *   ERR_CHOLESKY      any factorisation of the filter's chain, Sigma^s_s, S or Sigma~_n fails -- unlike the smoother a failed
 *                     chain step REFUSES the sample: the cross-covariance is broken;
 *   WARN_MEAN_NOCONV; REJECTED_GATE (z_pred, S, innov, maha, loglik are still written);
 *   SKIPPED_SMALL_DT / ERR_NEG_DT / ERR_DT_TOO_LARGE of gated dt[c], as an OR over the filter's chain.
 * A filter that commits nothing keeps every bit and gets NaN in its float outputs (mu_out / cov_out of a gated-out sample too);
 * it never changes a bit of another filter.  Stream-ordered, joins split streams, no host synchronisation, no allocation at
 * call time; one kernel serves every lanes_per_filter setting; fp32 engines compute in fp32, with wide_arithmetic in fp64.
 * Device groups: per shard through ukfb_group_shard. */
#define UKFB_DELAYED_MAX_STEPS 33
typedef struct ukfb_delayed_in {
    int steps;                    /* window length, step steps - 1 is the present                                        */
    const double* dt;             /* HOST [steps - 1]                                                                      */
    int slots, first_slot;
    const void* mu_hist_dev;      /* [slots][capacity][S]                                                                  */
    const void* cov_hist_dev;     /* [slots][capacity][PK]                                                                 */
    const void* in_a_dev;         /* [slots][capacity][3] or NULL                                                          */
    const void* in_b_dev;
    int lag_uniform;
    const int32_t* lag_dev;       /* [capacity] or NULL: lag_uniform                                                       */
    int meas_model_uniform;
    const int32_t* meas_model_dev; /* [capacity] or NULL: meas_model_uniform                                               */
    const void* z_dev;            /* [capacity][3]                                                                         */
    const void* Q_dev;            /* [capacity][9], or [9] with q_is_uniform                                               */
    int q_is_uniform;
} ukfb_delayed_in;
typedef struct ukfb_delayed_out { /* device pointers, engine precision; any may be NULL                                    */
    void* z_pred;                 /* [capacity][4]                                                                         */
    void* S;                      /* [capacity][9]                                                                         */
    void* innov;                  /* [capacity][3]                                                                         */
    void* maha;                   /* [capacity]                                                                            */
    void* loglik;                 /* [capacity]                                                                            */
    uint32_t* status;             /* [capacity]                                                                            */
    void* mu_out;                 /* [capacity][S]                                                                         */
    void* cov_out;                /* [capacity][PK]                                                                        */
} ukfb_delayed_out;
int ukfb_update_delayed_dev(ukfb_engine* e, const ukfb_delayed_in* in, int commit, const ukfb_delayed_out* out);
/* Host arrays of doubles, window order: mu_hist [steps][capacity][S], cov_hist [steps][capacity][D][D] (step steps - 1 is not
 * read), in_a / in_b [steps][capacity][3] or NULL; lag [capacity] or NULL (lag_uniform); meas_model_per_filter [capacity] or
 * NULL; z [capacity][3], Q [capacity][3][3].  Outputs (any may be NULL): z_pred [capacity][4], S [capacity][9], innov
 * [capacity][3], maha, loglik, status [capacity], mu_out [capacity][S], cov_out [capacity][D][D].  Synchronises. */
int ukfb_update_delayed(ukfb_engine* e, int steps, const double* dt, const double* mu_hist, const double* cov_hist, const double* in_a,
                        const double* in_b, int lag_uniform, const int32_t* lag, int meas_model, const int32_t* meas_model_per_filter,
                        const double* z, const double* Q, int commit, double* z_pred, double* S, double* innov, double* maha,
                        double* loglik, uint32_t* status, double* mu_out, double* cov_out);
/* The lag of a sample from its time stamp: step_ts_us (HOST, `steps` strictly increasing stamps of the window's steps, by value,
 * 1 <= steps <= UKFB_DELAYED_MAX_STEPS), sample_ts_us_dev [capacity] (int64) -> lag_out_dev [capacity] (int32): l = n - c*, c* the
 * step whose stamp is nearest the sample's (ties go to the OLDER step); a sample newer than step n gives 0; a sample older than
 * step 0 by more than half of step_ts[1] - step_ts[0] gives `steps`, which ukfb_update_delayed_dev reports as out of the
 * window.  The residual offset inside a step interval is ignored.  Stream-ordered. */
int ukfb_delayed_lag_dev(ukfb_engine* e, int steps, const int64_t* step_ts_us, const int64_t* sample_ts_us_dev, int32_t* lag_out_dev);

/* ---- relative measurements (odometry and scan-match increments between a step of this ring and the present, on the same
 * window and lags): ukf_batch_relative.h, a header of its own beside this one. */
/* ---- late SENSOR-FRAME samples (ids 0 ... 7 of enum ukfb_sensor_model through the same ring): ukf_batch_delayed_sensor.h. */

/* ---- forecast: read-only multi-step prediction into a ring ------------------------------------------------------------------ */
/* Where every filter will be after the next 1 ... steps predictions, with covariance, WITHOUT committing them (collision
 * checks, gating a scan that has not arrived yet, latency-compensated output at one common time for filters whose last samples
 * have different stamps, a planner's horizon): the smoother's mirror image.
 * A FORECAST RING has the history's format: mu_out_dev [slots][capacity][S], cov_out_dev [slots][capacity][PK] (packed lower
 * triangle, as ukfb_device_views), engine precision.  Step c (0 ... steps - 1) is the state after c + 1 predictions and lives
 * in slot (first_slot + c) % slots, so its records are valid inputs, as they lie, to ukfb_update_state_dev (commit = 0: the
 * distance between tracks at the horizon), ukfb_smooth_dev's conventions and ukfb_bank_combine_dev's records as a start.
 * in_a_dev / in_b_dev: optional input rings [slots][capacity][3] indexed like the forecast ring (the slot of step c = the
 * inputs of the prediction that PRODUCES step c), with the meaning they have in ukfb_cycle_multi_dev, the per-filter NaN
 * acceleration row that selects PoseUKF's constant-velocity branch included; NULL: the engine's latched inputs, held over the
 * horizon.  The chain starts from the START RECORD: start_mu_dev [capacity][S] and start_cov_dev [capacity][PK], both NULL (the
 * engine's own state) or both non-NULL (exactly one NULL: UKFB_ERR_INVALID_ARG).
 *
 * Each prediction is made exactly as ukfb_predict makes it (noise shaping and the acceleration-branch rule of
 * PoseUKF.cpp:188-193, mean_tol / mean_max_iter included) with the engine's process noise (batch-uniform or per filter),
 * acc.cov, taus and earth rotation at the time of the call: L = chol(Sigma), sigma points X_i, Y_i = g(X_i), the iterated mean
 * mu^-, delta_i = Y_i (-) mu^-, Sigma^- = 1/2 sum_i delta_i delta_i^T + R.  The time step of step c:
 *   dt form     every filter predicts by dt[c] (HOST, steps entries, passed to the kernel by value); the gate is
 *               ukfb_predict's own;
 *   ts_us form  what `steps` calls of predictionStepFromSampleTime(ts_us[c]) (UnscentedKalmanFilter.hpp:83-100; HOST, by
 *               value) would do to a COPY of the filter: each filter starts from ITS OWN last measurement time, read on the
 *               device, dt = double(ts - last) / 1000000.0 as the forward kernel computes it, and the copy's (shadow) last time
 *               advances only where it was null or dt > min_time_delta.  The engine's stored times are not written.
 * Exactly one of dt / ts_us is non-NULL (else UKFB_ERR_INVALID_ARG).  1 <= steps <= min(slots, UKFB_FORECAST_MAX_STEPS); a
 * larger steps is UKFB_ERR_OUT_OF_RANGE and writes nothing.  A longer horizon is chained by the caller: the next call starts
 * from the last slot of the previous one through start_*_dev (that needs cov_out_dev).
 * Status of the call, written to the caller's array ([capacity], may be NULL) as the OR over the steps:
 *   SKIPPED_FIRST_TS  (ts_us form) the filter's last measurement time is null: no prediction, the shadow time becomes ts_us[c];
 *   SKIPPED_SMALL_DT / ERR_NEG_DT / ERR_DT_TOO_LARGE  the step is gated (<= min_time_delta, < 0, > max_time_delta);
 *                     a step without a prediction receives the bits of the record before it, step 0 those of the start record;
 *   ERR_CHOLESKY      the chain's covariance cannot be factorised at a step: the step receives the previous record's bits and
 *                     the chain goes on from it;
 *   WARN_MEAN_NOCONV  the mean iteration hit its cap (mean_max_iter); the last iterate is used;
 *   UNINITIALISED     nothing is written for that filter.
 * A filter that fails, is gated or is uninitialised never changes a bit of another filter.  The calls are READ-ONLY on the
 * engine: mean, covariance, initialised flags, last measurement times, latches, noise and the engine's own status array keep
 * every bit (the kernel holds no pointer through which it could store to them).
 * Between the steps the chain stays in LDS in the arithmetic type; every record is narrowed to the storage type once, at its
 * store.  mu_out_dev / cov_out_dev must not alias the start record's memory, unless the start record is a slot of those rings
 * OUTSIDE the window (the chained call above).  Stream-ordered; joins split streams like every other call; no host
 * synchronisation, no allocation at call time.  The same kernel serves every lanes_per_filter setting; fp32 engines compute in
 * fp32, with wide_arithmetic in fp64 (stored fp32).  Device groups: per shard through ukfb_group_shard. */
#define UKFB_FORECAST_MAX_STEPS 32
int ukfb_forecast_dev(ukfb_engine* e, int steps, const double* dt, const int64_t* ts_us, int slots, int first_slot,
                      const void* start_mu_dev, const void* start_cov_dev, const void* in_a_dev, const void* in_b_dev,
                      void* mu_out_dev, void* cov_out_dev, uint32_t* status_dev);
/* host arrays of doubles in window order: start_mu [capacity][S] and start_cov [capacity][D][D] (both NULL: the engine's
 * state); in_a / in_b [steps][capacity][3] or NULL (the latched inputs); mu [steps][capacity][S], cov [steps][capacity][D][D]
 * (may be NULL) and status [capacity] (may be NULL) receive the forecast (zeros for an UNINITIALISED filter);
 * steps <= UKFB_FORECAST_MAX_STEPS; synchronises */
int ukfb_forecast(ukfb_engine* e, int steps, const double* dt, const int64_t* ts_us, const double* start_mu,
                  const double* start_cov, const double* in_a, const double* in_b, double* mu, double* cov, uint32_t* status);

/* ---- filter lifecycle: gather, scatter, retire, compact -------------------------------------------------------------------- */
/* Birth, death, clone, move and defragmentation of filters ON THE DEVICE: the whole per-filter record -- mean, packed
 * covariance, initialised flag, last measurement time, latched inputs, per-filter process noise -- read and written as a unit.
 * All four device calls are stream-ordered on the engine's stream (split launches are joined first), need no host
 * synchronisation and allocate nothing after an engine's first lifecycle call (that call creates one workspace, freed by
 * ukfb_destroy).  A NULL engine is UKFB_ERR_INVALID_ARG.  Lists on the device are int32 filter indices, like the lists of
 * ukfb_process_events_dev's rounds; scalars are in the engine's precision.  Device groups: per shard through ukfb_group_shard.
 *
 * A RECORD SET is n records in item order, field by field (ukfb_filter_records); a NULL field is skipped.
 * index_dev [n] names the filter of every item; NULL: item k is filter k.  n < 0 or n > INT32_MAX is UKFB_ERR_OUT_OF_RANGE,
 * n == 0 is UKFB_OK and launches nothing.  Item k is INVALID when index[k] < 0 or index[k] >= capacity (with a NULL index_dev:
 * k >= capacity); an invalid item is refused per item, never an error of the call.
 *
 * ukfb_gather_filters_dev is READ-ONLY on the engine: state, flags, times, latches, noise and the engine's own status array keep
 * every bit.  A valid item writes every non-NULL field of record k from filter index[k]: in_a / in_b are what that filter's next
 * prediction would read (the bound buffer if one is bound, else the engine's latch); noise is the filter's matrix (the uniform
 * matrix on an engine with batch-uniform noise); status[k] = 0.  An invalid item writes zeros to every field, initialised 0, and
 * status[k] = UKFB_ST_INACTIVE.  Duplicate indices are fine.
 *
 * ukfb_scatter_filters_dev is initializeFilter (UnscentedKalmanFilter.hpp:40-44) from device records.  mu and cov_packed are
 * required (else UKFB_ERR_INVALID_ARG).  A valid item writes mean and covariance as given -- nothing about them is checked, as in
 * ukfb_initialize; a covariance that cannot be factorised is reported by the first prediction.  The flag becomes
 * initialised[k] != 0 (a NULL field: 1) and the last measurement time last_ts_us[k] (a NULL field: 0, as initializeFilter
 * zeroes it); a record with initialised[k] == 0 RETIRES the filter: flag 0, time 0.  in_a / in_b, if given, go into the
 * engine-owned latch arrays (a bound buffer stays the caller's).  noise, if given, goes into the filter's per-filter entry: the
 * engine must ALREADY store its noise per filter (ukfb_set_process_noise_per_filter), otherwise the call is
 * UKFB_ERR_INVALID_ARG and writes nothing -- no storage is switched at call time; on Pose engines the filter's
 * acceleration-branch matrix (block (6,6,3,3) replaced by 2 acc.cov, PoseUKF.cpp:190-191) is rebuilt in the same call with the
 * bits ukfb_pose_set_acceleration would give.  The engine's own status word of the filter is not written.
 * DUPLICATES ARE DECIDED, NOT RACED: among the valid items that name the same filter the LOWEST item index wins and writes the
 * whole record (mean and covariance of a filter always come from the same item); every other such item writes nothing and gets
 * status[k] = UKFB_ST_INACTIVE, as does an invalid item; a winner gets 0.  Filters that no winning item names keep every bit.
 * The cost of a call follows n, not the capacity.  The records must not overlap the engine's own arrays.
 *
 * ukfb_retire_dev: every filter with a non-zero byte in retire_mask_dev [capacity] gets flag 0 and last measurement time 0; its
 * mean, covariance and everything else, and every other filter, keep their bits.  A later cycle reports UKFB_ST_UNINITIALISED
 * for it until a scatter (or ukfb_initialize) gives the slot a new filter.
 *
 * ukfb_compact_dev moves the live filters to the front IN PLACE, in groups of `group` consecutive filters: group = 1, or a bank's
 * M, so that the hypotheses t * M + j of a track stay together (1 <= group <= 8, capacity % group == 0, else
 * UKFB_ERR_INVALID_ARG).  With G = capacity / group, group g is LIVE if any of its filters is initialised and L is the number of
 * live groups.  The HOLES are the dead groups g < L in ascending order h_0 < h_1 < ..., the MOVERS the live groups g >= L in
 * ascending order m_0 < m_1 < ... (there are exactly as many): mover m_k is copied onto hole h_k, filter by filter -- mean and
 * packed covariance, flag and last measurement time, the engine's status word, the engine-owned in_a / in_b latches and, when
 * the noise is per filter, its process-noise and acceleration-branch entries -- and then the mover's flags are cleared and its
 * times set to 0; its other bits stay.  Nothing else changes: live groups below L and dead groups at or above L keep every bit,
 * and no buffer is reallocated or swapped, so the pointers of ukfb_device_views stay valid.  The mapping is fully determined by
 * the flags.  Outputs on the device, each may be NULL:
 *   new_index_dev [capacity]  for every filter i of a group that was live before the call its index after the call (i itself
 *                             if it did not move), -1 for every other filter;
 *   old_index_dev [capacity]  for j < L * group the index that filter had before the call, -1 for j >= L * group;
 *   live_dev      [1]         L * group: the free slots start here, so that births need no host -- a caller forms
 *                             index = live + arange(n) on the device and scatters; items beyond the capacity are refused per item.
 * BOUND input buffers (ukfb_pose_bind_acceleration_dev, ukfb_orient_bind_inputs_dev) and every other per-filter array of the
 * caller are the caller's: they are NOT moved, the caller permutes them with old_index_dev.  ukfb_last_model_groups refers to
 * the numbering before the call.  A filter that moves gets other wave-mates: later results agree to rounding with those of the
 * uncompacted engine, bit for bit only where placement is the same (the reproducibility rule at the top of this file). */
typedef struct ukfb_filter_records {   /* device pointers, n records in item order; any may be NULL unless said otherwise */
    void*     mu;           /* [n][S]                                                             */
    void*     cov_packed;   /* [n][PK]  packed lower triangle, as ukfb_device_views               */
    int64_t*  last_ts_us;   /* [n]                                                                */
    uint8_t*  initialised;  /* [n]                                                                */
    void*     in_a;         /* [n][3]   Pose acc.mu / Orient acceleration.mu                      */
    void*     in_b;         /* [n][3]   Orient rotation_rate.mu                                   */
    void*     noise;        /* [n][D][D] row-major process noise                                  */
    uint32_t* status;       /* [n]      UKFB_ST_* of THIS call, per item                          */
} ukfb_filter_records;
int ukfb_gather_filters_dev(ukfb_engine* e, int64_t n, const int32_t* index_dev, const ukfb_filter_records* out);
int ukfb_scatter_filters_dev(ukfb_engine* e, int64_t n, const int32_t* index_dev, const ukfb_filter_records* in);
int ukfb_retire_dev(ukfb_engine* e, const uint8_t* retire_mask_dev /* [capacity] */);
int ukfb_compact_dev(ukfb_engine* e, int group, int32_t* new_index_dev, int32_t* old_index_dev, int64_t* live_dev);
/* host-array forms (doubles, full D x D covariances; index [n] host int32 or NULL; any output may be NULL; scatter: mu and cov
 * required, last_ts_us / initialised / status may be NULL); they synchronise */
int ukfb_gather_filters(ukfb_engine* e, int64_t n, const int32_t* index, double* mu, double* cov, int64_t* last_ts_us,
                        uint8_t* initialised);
int ukfb_scatter_filters(ukfb_engine* e, int64_t n, const int32_t* index, const double* mu, const double* cov,
                         const int64_t* last_ts_us, const uint8_t* initialised, uint32_t* status);
int ukfb_compact(ukfb_engine* e, int group, int32_t* new_index, int32_t* old_index, int64_t* live);

/* ---- joint state-block measurements: update and fuse with full covariance ------------------------------------------------ */
/* ukf->update(z, h, Q) with z a SUB-MANIFOLD of the state and h the selection of blocks: a 6-DOF pose with its joint
 * covariance as ONE measurement, another estimate of the same state (a second engine's ukfb_device_views, a history slot, a
 * record of ukfb_bank_combine_dev) fused as information, with covariance intersection where the two are correlated to an
 * unknown degree, and the D-dimensional Mahalanobis distance / likelihood between a filter and a full estimate.
 * BLOCKS in host-layout order, one bit each:
 *   Pose              bit 0 position, bit 1 orientation, bit 2 velocity, bit 3 angular velocity;
 *   OrientationState  bit 0 orientation, bit 1 velocity, bit 2 bias_gyro, bit 3 bias_acc, bit 4 gravity.
 * A mask selects m = sum of the block dimensions tangent dimensions; the measurement manifold is the compound of the selected
 * blocks in state order.  z_dev [capacity][S] is a measurement in the STATE'S OWN LAYOUT: entries of unselected blocks are never
 * read and may be NaN; a selected quaternion is taken as given, as the state's is.  Qz_packed_dev [capacity][PK] is the packed
 * lower triangle of a D x D matrix in the state's tangent order (the format of ukfb_device_views); only rows and columns of
 * selected dimensions are read.  So a record of ukfb_device_views, a history slot or ukfb_bank_combine_dev is a valid
 * measurement as it lies.  block_mask_dev: int32 [capacity], or NULL so that block_mask_uniform serves every filter.  A
 * per-filter mask <= 0 or with bits beyond the model's blocks: no measurement for that filter (untouched, INACTIVE); such a
 * uniform mask is UKFB_ERR_INVALID_ARG.
 * state_inflation = a >= 1 and meas_inflation = b >= 1 (HOST, by value; below 1 or non-finite: UKFB_ERR_INVALID_ARG): the update
 * runs on a Sigma and b Qz.  1, 1 is the Kalman update (the multiplication by 1.0 is exact); a = 1 / w, b = 1 / (1 - w) is
 * covariance intersection with weight w.
 * Per filter with a valid mask ((+) / (-): the engine's; sel = the selected tangent dimensions):
 *   1. L = chol(a Sigma), sigma points X_i, Z_i = the selected blocks of X_i;
 *   2. z-bar = the iterated mean of the Z_i on the measurement manifold (start Z_0, mean_tol / mean_max_iter);
 *   3. S = 1/2 sum dz_i dz_i^T + b Qz[sel][sel], C = 1/2 sum (X_i (-) mu) dz_i^T (D x m; X_j+- (-) mu = +-L col j, which the
 *      kernel uses);
 *   4. S = Ls Ls^T; Y = C Ls^-T (one triangular solve per row), so that K = Y Ls^-1 and K S K^T = Y Y^T;
 *   5. nu = z (-) z-bar, y = Ls^-1 nu, d^2 = nu^T S^-1 nu = |y|^2, ln det S = sum ln of the pivots;
 *   6. the gate of ukfb_update_dev (gate_chi2 < 0: accept; else d^2 <= gate_chi2): REJECTED_GATE keeps the state, maha and
 *      loglik are still written;
 *   7. Sigma~ = a Sigma - Y Y^T;
 *   8. (mu, Sigma) = applyDelta(mu, Sigma~, Y y), the update's own commit.
 * commit = 1: an update like ukfb_update_dev, mean, covariance and the engine's own status array are written.  commit = 0:
 * READ-ONLY like ukfb_innovation_dev -- mean, covariance, times, latches, noise and the engine's status keep every bit, only
 * `out` is written (the same numbers: every step above still runs).
 * Status of THIS call (out->status, and with commit = 1 the engine's status array):
 *   UNINITIALISED       the filter is uninitialised;
 *   INACTIVE            no valid mask for this filter;
 *   ERR_NONFINITE_MEAS  a SELECTED entry of z or Qz is non-finite;
 *   ERR_CHOLESKY        a Sigma, S or (an accepted update's) Sigma~ is not positive definite;
 *   WARN_MEAN_NOCONV    the mean iteration hit its cap;
 *   REJECTED_GATE       the gate rejected the update.
 * A filter with one of the first four keeps its state bit for bit and writes NaN to maha / loglik; it never changes a bit of
 * another filter.  Stream-ordered, no host synchronisation, no allocation at call time.  The same kernel serves every
 * lanes_per_filter setting; fp32 engines compute in fp32, with wide_arithmetic in fp64 (stored fp32).  Device groups: per shard
 * through ukfb_group_shard. */
#define UKFB_BLOCK_POSE_POSITION 1u
#define UKFB_BLOCK_POSE_ORIENTATION 2u
#define UKFB_BLOCK_POSE_VELOCITY 4u
#define UKFB_BLOCK_POSE_ANGULAR_VELOCITY 8u
#define UKFB_BLOCK_POSE_ALL 15u
#define UKFB_BLOCK_ORIENT_ORIENTATION 1u
#define UKFB_BLOCK_ORIENT_VELOCITY 2u
#define UKFB_BLOCK_ORIENT_BIAS_GYRO 4u
#define UKFB_BLOCK_ORIENT_BIAS_ACC 8u
#define UKFB_BLOCK_ORIENT_GRAVITY 16u
#define UKFB_BLOCK_ORIENT_ALL 31u
typedef struct ukfb_state_meas_out {   /* device pointers, engine precision; any may be NULL */
    void*     maha;     /* [capacity]  d^2 = nu^T S^-1 nu over the m selected dimensions          */
    void*     loglik;   /* [capacity]  -0.5 (d^2 + ln det S + m ln 2 pi)                          */
    uint32_t* status;   /* [capacity]  UKFB_ST_* of THIS call                                     */
} ukfb_state_meas_out;
/* out may be NULL with commit = 1 */
int ukfb_update_state_dev(ukfb_engine* e, uint32_t block_mask_uniform, const int32_t* block_mask_dev,
                          const void* z_dev, const void* Qz_packed_dev,
                          double state_inflation, double meas_inflation, int commit,
                          const ukfb_state_meas_out* out);
/* host arrays of doubles: z [capacity][S], Qz [capacity][D][D] (the lower triangle is read), block_mask_per_filter [capacity]
 * or NULL; maha / loglik / status [capacity], any may be NULL; synchronises */
int ukfb_update_state(ukfb_engine* e, uint32_t block_mask, const int32_t* block_mask_per_filter /* or NULL */,
                      const double* z, const double* Qz, double state_inflation, double meas_inflation, int commit,
                      double* maha, double* loglik, uint32_t* status);
/* Pose engines only (else UKFB_ERR_WRONG_MODEL): base::samples::RigidBodyState records (the 49 scalars of
 * ukfb_pose_export_body_states) integrated as measurements.  z = the record's fields AS THEY ARE (no inverse rotation of the
 * velocity, as fromRigidBodyState and ukfb_pose_import_body_states), Qz = the four 3 x 3 blocks on the diagonal; inflation 1, 1,
 * commit = 1.  active [capacity] or NULL: a filter with active == 0 gets no measurement (INACTIVE).  Synchronises. */
int ukfb_pose_update_body_states(ukfb_engine* e, uint32_t block_mask, const double* records /* [capacity][49] */,
                                 const uint8_t* active /* or NULL */);

/* ---- sensor-frame measurements: lever arms, ranges and landmark fixes ---------------------------------------------------- */
/* ukf->update(z, h, Q) for sensors that are NOT at the body origin or not aligned with the body: h is nonlinear in the
 * orientation (and, with a lever arm, couples the sample to the angular velocity), and the sigma points carry that coupling
 * into the update -- which rotating and shifting the sample into the body frame with the current mean, before an update with
 * a state-selecting model, discards.  The measurement space is R^m, m = 1 or 3.  q = the state's orientation (body -> nav),
 * R(q) x = the rotation of x by q (Eigen's _transformVector), R(q)^T x = the rotation by q^-1 = conj(q) / |q|^2.
 * MOUNT = r[3], the sensor's origin in the body frame, then qs[4] (x, y, z, w), the sensor -> body rotation; POINT = b[3], a
 * nav-frame vector.  qs is taken as given, as the state's quaternion is.
 *   id  engine  m  h(X)
 *   0   Pose    3  p + R(q) r                                  antenna with a lever arm
 *   1   Pose    1  | (p - b) + R(q) r |                        range to a beacon at b
 *   2   Pose    3  R(qs)^T (R(q)^T (b - p) - r)                a known point seen in the sensor frame (USBL, landmark)
 *   3   Pose    3  R(qs)^T (v + omega x r)                     velocity at the sensor, sensor frame (v, omega: body frame)
 *   4   Pose    3  R(q) v                                      nav-frame velocity
 *   5   Orient  3  R(qs)^T (R(q)^T v + (w_gyro - b_g) x r)     the same for OrientationState; w_gyro = the latched gyro input
 *   6   Orient  3  R(qs)^T R(q)^T b                            a nav-frame direction seen from the sensor (magnetometer, sun)
 *   7   Orient  3  R(q)^T (0, 0, g) + b_a                      accelerometer at rest (g, b_a from the state)
 * A model reads only what its h names: POSITION / RANGE r; POINT r, qs; the VELOCITY models r, qs; NAV_VECTOR qs; and b where
 * it appears.  Entries a model does not read -- z[m ...], Q outside the leading m x m, the rest of mount / point -- are never
 * used and may be NaN.  A negative per-filter id: no measurement for that filter (untouched, INACTIVE); so is an id of the
 * other engine's models or beyond 7.  Such a UNIFORM id is UKFB_ERR_WRONG_MODEL.
 * Per filter the steps are those of ukf::update:
 *   1. L = chol(Sigma), sigma points X_i, Z_i = h(X_i);
 *   2. z-bar = the iterated mean from Z_0 (mean_tol / mean_max_iter; on a vector space it moves once and confirms);
 *   3. S = 1/2 sum dz_i dz_i^T + Q;  C = 1/2 sum (X_i (-) mu) dz_i^T  (D x m; X_j+- (-) mu = +-L col j, which the kernel uses);
 *   4. S = Ls Ls^T; Y = C Ls^-T, so that K = Y Ls^-1 and K S K^T = Y Y^T;
 *   5. nu = z - z-bar, y = Ls^-1 nu, d^2 = nu^T S^-1 nu = |y|^2, ln det S = sum ln of the pivots;
 *   6. the gate of ukfb_update_dev (gate_chi2 < 0: accept; else d^2 <= gate_chi2): REJECTED_GATE keeps the state, the outputs
 *      are still written;
 *   7. Sigma~ = Sigma - Y Y^T; (mu, Sigma) = applyDelta(mu, Sigma~, Y y), the update's own commit.
 * commit = 1: mean, covariance and the engine's own status array are written.  commit = 0: READ-ONLY like
 * ukfb_innovation_dev -- mean, covariance, times, latches, noise and the engine's status keep every bit, only `out` is written
 * (the same numbers: every step above still runs).
 * Status of THIS call (out->status, and with commit = 1 the engine's status array):
 *   UNINITIALISED       the filter is uninitialised;
 *   INACTIVE            no valid model id for this filter;
 *   ERR_NONFINITE_MEAS  a non-finite value among the first m of z, the leading m x m of Q or the mount / point entries the
 *                       filter's model reads;
 *   ERR_CHOLESKY        Sigma, S or (an accepted update's) Sigma~ is not positive definite;
 *   WARN_MEAN_NOCONV    the mean iteration hit its cap;
 *   REJECTED_GATE       the gate rejected the update.
 * A filter with one of the first four keeps its state bit for bit and writes NaN to its float outputs (padding entries: 0); it
 * never changes a bit of another filter.  Stream-ordered, no host synchronisation, no allocation at call time.  The same kernel
 * serves every lanes_per_filter setting; fp32 engines compute in fp32, with wide_arithmetic in fp64 (stored fp32).  Device
 * groups: per shard through ukfb_group_shard. */
enum ukfb_sensor_model {
    UKFB_SENSOR_NONE = -1,
    UKFB_SENSOR_POSE_POSITION = 0,
    UKFB_SENSOR_POSE_RANGE = 1,
    UKFB_SENSOR_POSE_POINT = 2,
    UKFB_SENSOR_POSE_VELOCITY = 3,
    UKFB_SENSOR_POSE_NAV_VELOCITY = 4,
    UKFB_SENSOR_ORIENT_VELOCITY = 5,
    UKFB_SENSOR_ORIENT_NAV_VECTOR = 6,
    UKFB_SENSOR_ORIENT_SPECIFIC_FORCE = 7
};
typedef struct ukfb_sensor_in {   /* device pointers in engine precision; the *_uniform values are host doubles, by value */
    const int32_t* model_dev;     /* [capacity] model id per filter, or NULL: the call's model_uniform serves every filter */
    const void*    z_dev;         /* [capacity][3]  the first m entries are read                                          */
    const void*    Q_dev;         /* [capacity][9] row-major 3x3, or ONE 3x3 with q_is_uniform; the lower triangle of the
                                     leading m x m block is what the factorisation reads (as ukfb_update_dev)             */
    int            q_is_uniform;
    const void*    mount_dev;     /* [capacity][7] r, then qs (x, y, z, w); NULL: mount_uniform serves every filter       */
    double         mount_uniform[7];
    const void*    point_dev;     /* [capacity][3]; NULL: point_uniform serves every filter                               */
    double         point_uniform[3];
} ukfb_sensor_in;
typedef struct ukfb_sensor_out {  /* device pointers, engine precision; any may be NULL                                  */
    void*     z_pred;   /* [capacity][3]  z-bar: first m entries (rest 0)                                                */
    void*     S;        /* [capacity][9]  row-major 3x3, leading m x m block = S, rest 0                                 */
    void*     innov;    /* [capacity][3]  nu = z - z-bar, first m entries (rest 0)                                       */
    void*     maha;     /* [capacity]     d^2 = nu^T S^-1 nu                                                             */
    void*     loglik;   /* [capacity]     -0.5 (d^2 + ln det S + m ln 2 pi)                                              */
    uint32_t* status;   /* [capacity]     UKFB_ST_* of THIS call                                                         */
} ukfb_sensor_out;
/* out may be NULL with commit = 1 */
int ukfb_update_sensor_dev(ukfb_engine* e, int model_uniform, const ukfb_sensor_in* in, int commit, const ukfb_sensor_out* out);
/* host arrays of doubles: z [capacity][3], Q [capacity][3][3]; model_per_filter [capacity] or NULL (then `model`); mount
 * [capacity][7] or NULL, then mount_uniform [7] (NULL: r = 0, qs the identity); point [capacity][3] or NULL, then point_uniform
 * [3] (NULL: 0).  z_pred [capacity][3], S [capacity][3][3], innov [capacity][3], maha / loglik / status [capacity]: any may be
 * NULL.  Synchronises. */
int ukfb_update_sensor(ukfb_engine* e, int model, const int32_t* model_per_filter /* or NULL */, const double* z, const double* Q,
                       const double* mount /* or NULL */, const double* mount_uniform /* or NULL */,
                       const double* point /* or NULL */, const double* point_uniform /* or NULL */, int commit,
                       double* z_pred, double* S, double* innov, double* maha, double* loglik, uint32_t* status);
/* ---- the robust form (an outlier is down-weighted by an inflated Q, not rejected): ukf_batch_robust.h, a header of its own. */

/* ---- bearing measurements: directions on the sphere S^2 ------------------------------------------------------------------ */
/* ukf->update(z, h, Q) for sensors that measure a DIRECTION: a camera pixel of a known landmark, a USBL or sonar bearing, a
 * sun or star sensor, a magnetometer whose magnitude is not trusted.  The measurement is a unit vector in the sensor frame, a
 * point of the manifold S^2 (ukfom: MTK::S2): its noise is two-dimensional, its mean is iterated on the sphere and its
 * differences are sphere logarithms.  Conventions (q, R(q) x, MOUNT = r[3], qs[4], POINT = b[3]) as for the sensor-frame
 * measurements above.  h(X) = d(X) / |d(X)| with
 *   id  engine  d(X)
 *   0   Pose    R(qs)^T (R(q)^T (b - p) - r)      the direction to a known point b
 *   1   Pose    R(qs)^T R(q)^T b                  a nav-frame direction b (sun, field)
 *   2   Orient  R(qs)^T R(q)^T b                  the same for OrientationState
 * POSE_POINT reads r, qs, b; the NAV_DIRECTION models qs, b.  Entries a model does not read may be NaN and never meet
 * arithmetic.  A negative per-filter id: no measurement for that filter (untouched, INACTIVE); so is an id of the other
 * engine's model or beyond 2.  Such a UNIFORM id is UKFB_ERR_WRONG_MODEL.
 * ukfb_sensor_in / ukfb_sensor_out are reused; what their fields mean HERE:
 *   z_dev   [capacity][3]  the measured direction; it need not be normalised, the call uses z^ = z / |z|
 *   Q_dev   [capacity][9] or ONE 3x3 with q_is_uniform: the covariance of the direction noise as a 3-vector in the sensor
 *           frame, symmetric, the lower triangle is read.  Only its tangent part at the predicted direction enters: P Q P with
 *           P = I - z-bar z-bar^T.  The caller never sees a tangent basis, and no result depends on one.
 *   z_pred  [capacity][3]  z-bar, a unit vector
 *   S       [capacity][9]  Sigma_z + P Q P: 3 x 3 of rank 2 in the ambient frame (S z-bar = 0), WITHOUT the z-bar z-bar^T term below
 *   innov   [capacity][3]  nu = log_z-bar(z^), nu perpendicular to z-bar
 *   maha    d^2 = nu^T S3^-1 nu;  loglik = -0.5 (d^2 + ln det S3 + 2 ln 2 pi)
 * Sphere maps, for unit u, v and w perpendicular to u:
 *   log_u(v) = theta t / |t|, t = v - (u.v) u, theta = atan2(|u x v|, u.v); exact zeros at v = u.  The result is tangent at u
 *              over the whole range, the neighbourhood of the antipode included: |u . log_u(v)| <= 8 eps |log_u(v)|, eps = 2^-52.
 *              Where the tangent part of v is not resolved (u.v < 0 and |t| <= 4 eps: theta within 4 eps of pi, the exact
 *              antipode included) a tangent vector of length pi: the direction is unspecified, the result finite.
 *   exp_u(w) = cos|w| u + sinc|w| w, renormalised.
 * Per filter the steps are those of ukf::update with the measurement manifold S^2:
 *   1. L = chol(Sigma), sigma points X_i, Z_i = h(X_i);
 *   2. z-bar = the iterated mean from Z_0: m = 1/(2 D + 1) sum_i log_ref(Z_i), ref <- exp_ref(m), until |m| <= mean_tol or
 *      mean_max_iter trips (WARN_MEAN_NOCONV); the step is applied before it is judged.  Unlike on R^m this really iterates;
 *   3. w_i = log_z-bar(Z_i); Sigma_z = 1/2 sum w_i w_i^T (3 x 3, Sigma_z z-bar = 0); C = 1/2 sum (X_i (-) mu) w_i^T (D x 3);
 *   4. S3 = Sigma_z + P Q P + z-bar z-bar^T: positive definite with a unit eigenvalue along z-bar; d^2, ln det S3 and
 *      K = C S3^-1 equal the 2 x 2 quantities in ANY orthonormal tangent basis B (S2 = B^T (Sigma_z + Q) B, ...), because S3 is
 *      block diagonal in (B, z-bar) and nu and the columns of C^T have no component along z-bar;
 *   5. nu = log_z-bar(z^), d^2 and loglik as above;
 *   6. the gate of ukfb_update_dev;
 *   7. Sigma~ = Sigma - Y Y^T (Y = C Ls^-T, S3 = Ls Ls^T); (mu, Sigma) = applyDelta(mu, Sigma~, K nu).
 * commit = 0, the status rules, NaN to the float outputs of a refused filter, "never changes a bit of another filter", stream
 * ordering, no allocation at call time and the fp32 / wide_arithmetic behaviour are those of ukfb_update_sensor_dev.  In
 * addition: ERR_NONFINITE_MEAS also covers |z|^2 zero or not finite (and here every entry of z and Q is judged); a sigma point
 * whose |d|^2 is zero or not finite (a landmark exactly at the sensor, b = 0) makes S non-finite: ERR_CHOLESKY, the state is
 * kept.  No new status bit. */
enum ukfb_bearing_model {
    UKFB_BEARING_NONE = -1,
    UKFB_BEARING_POSE_POINT = 0,           /* Pose    d = R(qs)^T (R(q)^T (b - p) - r)   direction to a known point        */
    UKFB_BEARING_POSE_NAV_DIRECTION = 1,   /* Pose    d = R(qs)^T R(q)^T b               a nav-frame direction (sun, field) */
    UKFB_BEARING_ORIENT_NAV_DIRECTION = 2  /* Orient  d = R(qs)^T R(q)^T b                                                  */
};
/* out may be NULL with commit = 1 */
int ukfb_update_bearing_dev(ukfb_engine* e, int model_uniform, const ukfb_sensor_in* in, int commit, const ukfb_sensor_out* out);
/* host arrays of doubles, shaped as for ukfb_update_sensor.  Synchronises. */
int ukfb_update_bearing(ukfb_engine* e, int model, const int32_t* model_per_filter /* or NULL */, const double* z, const double* Q,
                        const double* mount /* or NULL */, const double* mount_uniform /* or NULL */,
                        const double* point /* or NULL */, const double* point_uniform /* or NULL */, int commit,
                        double* z_pred, double* S, double* innov, double* maha, double* loglik, uint32_t* status);

/* ---- sensor-frame association: K candidates per filter in one launch ------------------------------------------------------ */
/* The sensor-frame measurements above (model ids 0 ... 7 of enum ukfb_sensor_model, the same h, steps and conventions) scored
 * against up to UKFB_ASSOCIATE_MAX_CANDIDATES candidate samples per filter, the nearest candidate inside the gate chosen, and
 * with commit = 1 the update finished with it: which of several USBL or sonar returns belongs to this track, which map
 * landmark a POSE_POINT fix refers to, which beacon a POSE_RANGE belongs to.  Two modes, one per call:
 *   point_per_candidate = 0  SHARED-H: K detections z[k] against one hypothesis (the point is per filter or uniform, as in
 *                            ukfb_sensor_in).  Steps 1 - 4 of ukfb_update_sensor_dev run once, step 5 per candidate.  H = 1.
 *   point_per_candidate = 1  PER-HYPOTHESIS: candidate k pairs z[k] with the landmark or beacon b[k].  Step 1 runs once,
 *                            steps 2 - 5 per candidate on the same sigma points.  H = candidates.  For a filter whose model
 *                            does not read b the flag has no effect (its H hypotheses are equal) and the points are never read.
 * A candidate is ABSENT when an entry among the first m of z[k] -- or, per-hypothesis, an entry of the b[k] its model reads --
 * is not finite: it scores NaN and is never best.  This is how a ragged detection list is padded.  A candidate whose own S is
 * not positive definite scores NaN and is never best.
 *   best     the candidate with the smallest finite d^2, with cfg.gate_chi2 >= 0 only among those with d^2 <= gate_chi2 (the
 *            update's own comparison); equal d^2: the lower index; -1: none (ukfb_innovation_dev's rule)
 *   n_gated  the number of finite candidates inside the gate (all finite ones when the gate is off): above 1 the association
 *            is ambiguous
 * commit = 1: steps 6 - 7 run with the best candidate's nu (per-hypothesis: and its Y, Ls); mean, covariance and the engine's
 * own status array are written.  commit = 0: READ-ONLY on the engine, bit for bit, like ukfb_innovation_dev.
 * Status of THIS call (out->status, and with commit = 1 the engine's status array):
 *   UNINITIALISED, INACTIVE, WARN_MEAN_NOCONV  as in ukfb_update_sensor_dev (per-hypothesis: any present candidate's mean);
 *   ERR_NONFINITE_MEAS  a non-finite Q or mount entry the model reads, or EVERY candidate is absent;
 *   ERR_CHOLESKY        Sigma fails, no present candidate has a positive-definite S, or the accepted update's Sigma~ fails;
 *   REJECTED_GATE       some candidate is finite and none is inside the gate; the scores are still written.
 * A filter with one of UNINITIALISED, INACTIVE, ERR_NONFINITE_MEAS, ERR_CHOLESKY keeps every bit, writes NaN to its float
 * outputs (padding entries of innov: 0) and -1 / 0 to best / n_gated; no filter ever changes a bit of another.  Stream-ordered,
 * no host synchronisation, no allocation at call time; the same kernel serves every lanes_per_filter setting; fp32 engines
 * compute in fp32, with wide_arithmetic in fp64 (stored fp32).  A uniform id of the other engine's models is
 * UKFB_ERR_WRONG_MODEL; candidates outside 1 ... 32 is UKFB_ERR_OUT_OF_RANGE and writes nothing.  Bearings on S^2, per-candidate
 * Q or mount and assignment across filters are not served; weighted association (the probabilistic data association update):
 * ukf_batch_pda.h, a header of its own; the one-to-one assignment across the filters of a scene, from the scores written
 * here: ukf_batch_assign.h, likewise.  Device groups: per shard through ukfb_group_shard. */
#define UKFB_ASSOCIATE_MAX_CANDIDATES 32
typedef struct ukfb_associate_in {   /* device pointers in engine precision; the *_uniform values are host doubles, by value */
    const int32_t* model_dev;        /* [capacity] model id per filter, or NULL: the call's model_uniform serves every filter */
    int            candidates;       /* K = 1 ... UKFB_ASSOCIATE_MAX_CANDIDATES                                               */
    const void*    z_dev;            /* [candidates][capacity][3]  the slot layout of ukfb_innovation_dev                     */
    const void*    Q_dev;            /* [capacity][9] row-major 3x3, or ONE 3x3 with q_is_uniform (as ukfb_sensor_in)         */
    int            q_is_uniform;
    const void*    mount_dev;        /* [capacity][7] r, then qs (x, y, z, w); NULL: mount_uniform serves every filter        */
    double         mount_uniform[7];
    const void*    point_dev;        /* point_per_candidate = 0: [capacity][3], or NULL: point_uniform serves every filter;
                                        point_per_candidate = 1: [candidates][capacity][3], not NULL                          */
    double         point_uniform[3];
    int            point_per_candidate;   /* 0: shared-h mode; 1: per-hypothesis mode                                         */
} ukfb_associate_in;
typedef struct ukfb_associate_out {  /* device pointers, engine precision; any may be NULL.  H: see above                     */
    void*     z_pred;   /* [H][capacity][3]           z-bar: first m entries (rest 0)                                         */
    void*     S;        /* [H][capacity][9]           row-major 3x3, leading m x m block = S, rest 0                          */
    void*     innov;    /* [candidates][capacity][3]  nu = z - z-bar, first m entries (rest 0)                                */
    void*     maha;     /* [candidates][capacity]     d^2 = nu^T S^-1 nu                                                      */
    void*     loglik;   /* [candidates][capacity]     -0.5 (d^2 + ln det S + m ln 2 pi)                                       */
    int32_t*  best;     /* [capacity]                                                                                         */
    int32_t*  n_gated;  /* [capacity]                                                                                         */
    uint32_t* status;   /* [capacity]                 UKFB_ST_* of THIS call                                                  */
} ukfb_associate_out;
/* out may be NULL with commit = 1 */
int ukfb_associate_sensor_dev(ukfb_engine* e, int model_uniform, const ukfb_associate_in* in, int commit, const ukfb_associate_out* out);
/* host arrays of doubles: z [candidates][capacity][3], Q [capacity][3][3]; model_per_filter, mount, mount_uniform as for
 * ukfb_update_sensor; point [capacity][3] (or, with point_per_candidate, [candidates][capacity][3]) or NULL, then point_uniform
 * [3] (NULL: 0).  Outputs shaped as in ukfb_associate_out: any may be NULL.  Synchronises. */
int ukfb_associate_sensor(ukfb_engine* e, int model, const int32_t* model_per_filter /* or NULL */, int candidates, const double* z,
                          const double* Q, const double* mount /* or NULL */, const double* mount_uniform /* or NULL */,
                          const double* point /* or NULL */, const double* point_uniform /* or NULL */, int point_per_candidate,
                          int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik, int32_t* best,
                          int32_t* n_gated, uint32_t* status);

/* ---- user-defined measurement models: sigma-point export, sampled update ------------------------------------------------- */
/* ukf->update(z, h, Q) for an h the library does not know (four DVL beams, a camera pixel of a known landmark, range plus
 * range rate, two antennas at once, ...).  The library hands out the sigma points of every filter, the caller evaluates h on
 * them with whatever they like (a torch expression, a kernel of their own), and the library finishes the update from the
 * samples Z_i = h(X_i) with the device functions, the commit, the statuses and the read-only mode of the built-in models.
 * The measurement space is R^m, m = 1 ... UKFB_SAMPLED_MAX_M, ONE m for the call (an angle goes in as a unit vector).
 *
 * LAYOUT: filter-major.  One filter's 2 D + 1 points are one contiguous record: X [capacity][2 D + 1][S], delta
 * [capacity][2 D + 1][D], Z [capacity][2 D + 1][m].  This departs ON PURPOSE from the slot-major rings of the multi-cycle,
 * history and forecast calls ([slots][capacity][...]): a caller's h is then an elementwise expression over the last axis with
 * two leading batch axes, and the four filters of a wavefront read one contiguous stretch.
 * POINT ORDER: ukfom's.  L = the lower Cholesky factor of Sigma; point 0 = mu, point 1 + 2 j = mu (+) L col j, point 2 + 2 j =
 * mu (+) (-L col j).  delta holds the tangent offsets themselves (0, +L col j, -L col j): a caller who wants h(mu (+) delta) in
 * a higher precision than the engine stores can form the points from these.
 *
 * ukfb_sigma_points_dev: READ-ONLY on the engine (mean, covariance, times, latches, noise and the engine's status array keep
 * every bit).  Point 0 is mu bit for bit.  status_dev [capacity] (may be NULL): 0, UNINITIALISED, or ERR_CHOLESKY (Sigma is not
 * positive definite); such a filter's rows of X and delta are NaN.  Either of X_out_dev / delta_out_dev may be NULL, not both.
 *
 * ukfb_update_sampled_dev, per active filter (the steps of the sensor-frame measurements with h replaced by a load):
 *   1. L = chol(Sigma): the same device function in the same order as the export, so that X_i (-) mu = +-L col j holds for the
 *      points the caller evaluated.  The X themselves are never read;
 *   2. z-bar = the iterated mean of the Z_i from Z_0 (mean_tol / mean_max_iter);
 *   3. S = 1/2 sum dz_i dz_i^T + Q;  C = 1/2 sum (X_i (-) mu) dz_i^T = sum_j (L col j) W_j^T;
 *   4. S = Ls Ls^T; Y = C Ls^-T;
 *   5. nu = z - z-bar, y = Ls^-1 nu, d^2 = |y|^2, ln det S from the pivots;
 *   6. the gate of ukfb_update_dev (gate_chi2): REJECTED_GATE keeps the state, the outputs are still written;
 *   7. Sigma~ = Sigma - Y Y^T; (mu, Sigma) = applyDelta(mu, Sigma~, Y y), the update's own commit.
 * THE STATE MUST NOT CHANGE BETWEEN THE EXPORT AND THE UPDATE: the samples belong to the sigma points of the state they were
 * exported from.  That is the caller's responsibility (as with the history ring of the delayed update); nothing checks it.
 * ARITHMETIC: the differences Z_i - Z_0 and z - Z_0 are formed first, in fp64, in every mode, and the mean iteration, S and nu
 * work on those differences.  The update is therefore invariant under a per-filter translation of z and all Z_i together
 * (only z_pred moves, by that translation).  A caller with an fp32 engine should write z and Z relative to an origin near the
 * values (h(mu), say) instead of storing tens of metres in fp32: the stored samples then resolve the deltas.
 * commit = 1: mean, covariance and the engine's own status array are written; out may be NULL.  commit = 0: READ-ONLY like
 * ukfb_innovation_dev, only `out` is written (the same numbers).
 * Status of THIS call (out->status, and with commit = 1 the engine's status array):
 *   UNINITIALISED       the filter is uninitialised;
 *   INACTIVE            active_dev says 0 for this filter;
 *   ERR_NONFINITE_MEAS  a non-finite value among z, the lower triangle of Q or any of the filter's (2 D + 1) m samples;
 *   ERR_CHOLESKY        Sigma, S or (an accepted update's) Sigma~ is not positive definite;
 *   WARN_MEAN_NOCONV    the mean iteration hit its cap;
 *   REJECTED_GATE       the gate rejected the update.
 * A filter with one of the first four keeps its state bit for bit and writes NaN to its float outputs; it never changes a bit
 * of another filter.  m outside 1 ... UKFB_SAMPLED_MAX_M: UKFB_ERR_OUT_OF_RANGE, nothing is written.  NULL in, Z_dev, z_dev or
 * Q_dev, or commit = 0 with nowhere to write: UKFB_ERR_INVALID_ARG.  Stream-ordered, joins split streams, no host
 * synchronisation, no allocation at call time.  The same kernel serves every lanes_per_filter setting; fp32 engines compute in
 * fp32, with wide_arithmetic in fp64 (stored fp32).  Device groups: per shard through ukfb_group_shard. */
#define UKFB_SAMPLED_MAX_M 6
int ukfb_sigma_points_dev(ukfb_engine* e, void* X_out_dev, void* delta_out_dev, uint32_t* status_dev);
typedef struct ukfb_sampled_in {
    int m;                      /* 1 ... UKFB_SAMPLED_MAX_M, one value for the call */
    const void* Z_dev;          /* [capacity][2D+1][m]  Z_i = h(X_i), the order of ukfb_sigma_points_dev */
    const void* z_dev;          /* [capacity][m] */
    const void* Q_dev;          /* [capacity][m][m] row-major, or ONE m x m with q_is_uniform; the lower triangle is read */
    int q_is_uniform;
    const uint8_t* active_dev;  /* [capacity] or NULL = all; 0: no measurement for that filter (INACTIVE) */
} ukfb_sampled_in;
typedef struct ukfb_sampled_out {   /* device, engine precision, any may be NULL */
    void* z_pred;  /* [capacity][m] */   void* S;      /* [capacity][m][m] */   void* innov; /* [capacity][m] */
    void* maha;    /* [capacity] */      void* loglik; /* [capacity] */         uint32_t* status; /* [capacity] */
} ukfb_sampled_out;
int ukfb_update_sampled_dev(ukfb_engine* e, const ukfb_sampled_in* in, int commit, const ukfb_sampled_out* out);
/* host arrays of doubles, synchronising: X [capacity][2D+1][S], delta [capacity][2D+1][D], status [capacity] (X or delta may be
 * NULL, not both; status may be NULL); Z [capacity][2D+1][m], z [capacity][m], Q [capacity][m][m] (ONE m x m with q_is_uniform),
 * active [capacity] or NULL; z_pred [capacity][m], S [capacity][m][m], innov [capacity][m], maha / loglik / status [capacity]:
 * any may be NULL */
int ukfb_sigma_points(ukfb_engine* e, double* X, double* delta, uint32_t* status);
int ukfb_update_sampled(ukfb_engine* e, int m, const double* Z, const double* z, const double* Q, int q_is_uniform,
                        const uint8_t* active, int commit, double* z_pred, double* S, double* innov, double* maha,
                        double* loglik, uint32_t* status);

/* ---- user-defined process models: predict from propagated sigma points ---------------------------------------------------- */
/* ukf->predict(f, R) for an f the library does not know (drag and thrusters, a coordinated turn, another bias model, any control
 * input).  The caller exports the sigma points (ukfb_sigma_points_dev), evaluates f on them with whatever they like and hands the
 * propagated points XX_i = f(X_i) back, in the export's layout and point order ([capacity][2 D + 1][S], filter-major); the
 * library finishes the prediction.  Per active, initialised filter:
 *   1. mu^- = the iterated mean of the XX_i, started at XX_0 (mean_tol / mean_max_iter, one count per move above the tolerance);
 *   2. Sigma^- = 1/2 sum (XX_i (-) mu^-)(XX_i (-) mu^-)^T + R.
 * R IS TAKEN AS GIVEN: [capacity][D][D] row-major (or ONE D x D with r_is_uniform), the lower triangle is read, the upper never.
 * There is no rotation into the body frame and no scaling by dt or dt^2; those belong to the built-in models'
 * predictionStepImpl, and a caller who wants them forms R that way.
 * NOTHING IS FACTORISED: the call reads neither Sigma nor its factor, the engine's covariance is only overwritten.  A filter
 * whose export reported ERR_CHOLESKY has rows of NaN and is caught here as ERR_NONFINITE_MEAS.
 * TIMES ARE NOT TOUCHED: last measurement times, noise tables, input bindings and latches keep every bit.  The caller knows the
 * dt they evaluated f with; a filter whose step the time gate would have skipped is passed active = 0, and a caller who tracks
 * stamps in the engine advances them with ukfb_set_last_measurement_time.
 * QUATERNION BLOCKS ARE USED AS GIVEN (unit to the rounding of the storage type; ukfom does not renormalise, neither does this).
 * ARITHMETIC: the differences XX_i - XX_0 of every vector block are formed first, in fp64, in every mode; the mean iteration
 * and the deltas of those blocks work on the differences, and the committed vector blocks are XX_0 + the mean difference.  The
 * call is therefore invariant under a per-filter translation of a vector block of all XX_i together (only that block of mu^-
 * moves).
 * commit = 1: mean, covariance and the engine's own status array are written; out may be NULL.  commit = 0: READ-ONLY like
 * ukfb_innovation_dev, only `out` is written (the same numbers).
 * Status of THIS call (out->status, and with commit = 1 the engine's status array):
 *   UNINITIALISED       the filter is uninitialised;
 *   INACTIVE            active_dev says 0 for this filter;
 *   ERR_NONFINITE_MEAS  a non-finite value among the filter's (2 D + 1) S samples or in the lower triangle of its R;
 *   WARN_MEAN_NOCONV    the mean iteration hit its cap (the prediction is still made).
 * A filter with one of the first three keeps its state bit for bit and writes NaN to its float outputs; it never changes a bit
 * of another filter.  NULL in, XX_dev or R_dev, commit outside 0 / 1, or commit = 0 with nowhere to write:
 * UKFB_ERR_INVALID_ARG, nothing is written.  Stream-ordered, joins split streams, no host synchronisation, no allocation at
 * call time, capturable.  The same kernel serves every lanes_per_filter setting; fp32 engines compute in fp32, with
 * wide_arithmetic in fp64 (stored fp32).  Device groups: per shard through ukfb_group_shard. */
typedef struct ukfb_predict_sampled_in {
    const void* XX_dev;         /* [capacity][2D+1][S]  XX_i = f(X_i), layout and point order of ukfb_sigma_points_dev */
    const void* R_dev;          /* [capacity][D][D] row-major, or ONE D x D with r_is_uniform; the lower triangle is read */
    int r_is_uniform;
    const uint8_t* active_dev;  /* [capacity] or NULL = all; 0: no prediction for that filter (INACTIVE) */
} ukfb_predict_sampled_in;
typedef struct ukfb_predict_sampled_out {   /* device, engine precision, any may be NULL */
    void* mu;          /* [capacity][S] */
    void* cov_packed;  /* [capacity][PK], the packed lower triangle of ukfb_device_views / the forecast ring */
    uint32_t* status;  /* [capacity] */
} ukfb_predict_sampled_out;
int ukfb_predict_sampled_dev(ukfb_engine* e, const ukfb_predict_sampled_in* in, int commit, const ukfb_predict_sampled_out* out);
/* host arrays of doubles, synchronising: XX [capacity][2D+1][S], R [capacity][D][D] (ONE D x D with r_is_uniform), active
 * [capacity] or NULL; mu [capacity][S], cov [capacity][D][D] (full, symmetric), status [capacity]: any may be NULL */
int ukfb_predict_sampled(ukfb_engine* e, const double* XX, const double* R, int r_is_uniform, const uint8_t* active,
                         int commit, double* mu /* [capacity][S] */, double* cov /* [capacity][D][D] */, uint32_t* status);


/* ---- covariance conditioning: eigenvalue repair of failed filters -------------------------------------------------------- */
/* A filter whose covariance has stopped being positive definite reports ERR_CHOLESKY, keeps its state, and fails again at the
 * next call.  This call repairs such filters where they live, without a round trip to the host, and keeps the stored quaternion
 * on the unit sphere.  Per selected, initialised filter, with the batch-uniform variance floor v [D] > 0 and the correlation
 * eigenvalue floor eps, 0 < eps < 1:
 *   1. a non-finite entry in the lower triangle of Sigma: the filter cannot be repaired (ERR_CHOLESKY below);
 *   2. d_t = Sigma_tt if Sigma_tt >= v_t, else v_t (a comparison of stored numbers); s_t = sqrt(d_t);
 *   3. C_ij = Sigma_ij / (s_i s_j) for i != j, C_ii = 1: the conditioning is judged in the filter's own sigmas, a position block
 *      in m^2 and a gyro-bias block in (rad/s)^2 each on its own scale;
 *   4. C = V Lambda V^T by cyclic Jacobi; eig_min / eig_max = the smallest / largest eigenvalue of C as it came in;
 *   5. the filter is DEFICIENT iff a diagonal was raised in step 2 or eig_min < eps / 2, else HEALTHY: status 0, nothing of its
 *      state is written, its covariance output is its input bit for bit;
 *   6. a deficient filter gets C' = C + sum_{k: lambda_k < eps} (eps - lambda_k) v_k v_k^T (mathematically V max(Lambda, eps)
 *      V^T; in this additive form the healthy subspace is touched by the rounding of the correction only) and
 *      Sigma'_ij = s_i s_j C'_ij, formed as the lower triangle and stored packed (symmetric by construction); the diagonal is
 *      formed as d_i C'_ii with C'_ii = 1 + a sum of non-negative terms, so that it never rounds below the floor.  Status
 *      REPAIRED.  The eps / 2 trigger and the eps target make the call idempotent: a repaired filter is healthy at the next call
 *      (as long as no eigenvalue was below eps - 1: the diagonal of C' stays below 2);
 *   7. with renormalize_quaternion = 1 the orientation quaternion of the mean becomes q / |q|, computed in the kernel's compute
 *      type (|q|^2 as fma(q3, q3, fma(q2, q2, fma(q1, q1, q0 q0))), q_i * (1 / sqrt(|q|^2))).  RULE: a quaternion with
 *      | |q|^2 - 1 | <= 8 u, u the unit roundoff of the STORAGE type (2^-24 / 2^-53), is unit to the rounding of the storage
 *      type and keeps every bit (a unit quaternion rounded to storage is within 2 u, the fp32 evaluation of |q|^2 adds at most
 *      4 u; a renormalised one is within the rule, so the flag is idempotent too).  A zero or non-finite quaternion is treated
 *      like step 1.  A filter whose only change is the renormalisation also reports REPAIRED.  Nothing else of the mean is ever
 *      touched, and with the flag 0 the mean is not touched at all.
 * JACOBI: round-robin ordering (every pair once per sweep), at most 12 sweeps; converged = the off-diagonal Frobenius norm
 * (both triangles) is at most 4 D u in front of a sweep, u the unit roundoff of the compute type; a pair with |m_pq| <= u is
 * not rotated ((m_qq - m_pp) / (2 m_pq) would overflow).  A filter that has not converged after the 12th sweep is treated like
 * step 1.  tests/condition_reference.py is the same definition in NumPy.
 * CHOOSING eps: storing Sigma' moves the eigenvalues of its correlation matrix by up to about D u_storage (8e-7 in fp32, 1.4e-15
 * in fp64).  An eps meant to make the next factorisation succeed should sit two orders above that: 1e-4 for fp32 storage, 1e-10
 * for fp64.
 * commit = 1: the covariance of deficient filters, a renormalised quaternion and the engine's own status array are written; out
 * may be NULL.  commit = 0: READ-ONLY like ukfb_predict_sampled_dev (the kernel is launched without a pointer through which it
 * could store to the engine), only `out` is written, the same numbers.
 * Status of THIS call (out->status, and with commit = 1 the engine's status array):
 *   UNINITIALISED       the filter is uninitialised;
 *   INACTIVE            select_dev says 0 for this filter;
 *   ERR_NONFINITE_MEAS  an entry of var_floor_dev is non-finite or not > 0: every selected filter, nothing is conditioned;
 *   ERR_CHOLESKY        steps 1 and 7 and the sweep cap: the filter cannot be repaired;
 *   REPAIRED            the covariance (step 6) or the quaternion (step 7) was repaired.
 * A filter with one of the first four keeps its state bit for bit and writes NaN to its float outputs; a filter that commits
 * nothing never changes a bit of another filter.  Times, noise tables, input bindings and latches are not touched.
 * NULL in or var_floor_dev, eig_floor outside (0, 1) or non-finite, commit or renormalize_quaternion outside 0 / 1, or
 * commit = 0 with nowhere to write: UKFB_ERR_INVALID_ARG, nothing is written.  Stream-ordered, joins split streams, no host
 * synchronisation, no allocation at call time, capturable.  The same kernel serves every lanes_per_filter setting; fp32 engines
 * compute in fp32, with wide_arithmetic in fp64 (stored fp32).  Device groups: per shard through ukfb_group_shard. */
typedef struct ukfb_condition_in {
    const void* var_floor_dev;      /* [D] engine precision, the variance floor per tangent dimension.  The device call cannot read
                                       it without synchronising, so it is judged in the kernel: every entry must be finite and > 0,
                                       else every selected filter reports ERR_NONFINITE_MEAS and keeps its state (the sampled
                                       calls' treatment of a bad R) */
    double eig_floor;               /* epsilon, 0 < eps < 1 */
    const uint8_t* select_dev;      /* [capacity] or NULL = all; 0: the filter is not conditioned (INACTIVE) */
    int renormalize_quaternion;     /* 0 / 1 */
} ukfb_condition_in;
typedef struct ukfb_condition_out { /* device, engine precision, any may be NULL */
    void* eig_min;     /* [capacity]  of C as it came in */
    void* eig_max;     /* [capacity] */
    void* mu;          /* [capacity][S]  the mean after the call */
    void* cov_packed;  /* [capacity][PK] the covariance after the call, the packed lower triangle of ukfb_device_views */
    uint32_t* status;  /* [capacity] */
} ukfb_condition_out;
int ukfb_condition_dev(ukfb_engine* e, const ukfb_condition_in* in, int commit, const ukfb_condition_out* out);
/* host arrays of doubles, synchronising: var_floor [D] (an entry that is non-finite or not > 0: UKFB_ERR_INVALID_ARG before
 * anything is uploaded), select [capacity] or NULL; eig_min / eig_max [capacity], mu [capacity][S], cov [capacity][D][D] (full,
 * symmetric), status [capacity]: any may be NULL */
int ukfb_condition(ukfb_engine* e, const double* var_floor /* [D] */, double eig_floor, const uint8_t* select,
                   int renormalize_quaternion, int commit, double* eig_min, double* eig_max, double* mu,
                   double* cov /* [capacity][D][D] */, uint32_t* status);


/* ---- device groups: one host process, several MI355X ------------------------------------------------------------------ */
/* north_star's multi-GPU shape for a C++ host.  The filters of a batch are independent -- every filter of the reference owns
 * its own `ukf` object (src/UnscentedKalmanFilter.hpp:150) -- so `total_filters` split into contiguous shards (the first
 * total % n shards own one filter more; ukfb_group_shard_range), one engine with its own stream per device, and NO
 * collective on the data path.  The calls below fan out to the shards from the calling thread: the hot-path calls only
 * enqueue (the devices then run concurrently), ukfb_group_sync waits for all of them.  The one exchange is the result
 * gather, an RCCL all-gather of the means over xGMI.  Errors: the usual codes, text in ukfb_last_error().
 * `devices` may name a device more than once (several shards on one GPU: everything but the gather works). */
typedef struct ukfb_group ukfb_group;
int ukfb_group_shard_range(int64_t total, int n_shards, int shard, int64_t* first, int64_t* count);
int ukfb_group_create(ukfb_group** out, int model, int precision, int64_t total_filters, const int* devices, int n_devices);
int ukfb_group_destroy(ukfb_group* g);
int ukfb_group_size(const ukfb_group* g);   /* shards, -1 for NULL */
/* shard `shard`: its engine (every per-engine call above applies to it), device, first filter and filter count */
int ukfb_group_shard(ukfb_group* g, int shard, ukfb_engine** engine, int* device, int64_t* first, int64_t* count);
int ukfb_group_set_config(ukfb_group* g, const ukfb_config* cfg);
/* whole-batch host arrays, [first, first + count) in BATCH numbering, routed to the shards that own the filters */
int ukfb_group_initialize(ukfb_group* g, int64_t first, int64_t count, const double* mu, const double* cov);
int ukfb_group_get_state(ukfb_group* g, int64_t first, int64_t count, double* mu, double* cov, uint8_t* initialised);
int ukfb_group_get_status(ukfb_group* g, int64_t first, int64_t count, uint32_t* status);
int ukfb_group_get_status_summary(ukfb_group* g, uint32_t* or_of_all);
int ukfb_group_set_process_noise(ukfb_group* g, const double* R);
int ukfb_group_pose_set_acceleration(ukfb_group* g, int64_t first, int64_t count, const double* acc_mu, const double* acc_cov);
int ukfb_group_orient_set_params(ukfb_group* g, double gyro_bias_tau, double acc_bias_tau, const double earth_rotation[3]);
int ukfb_group_orient_set_inputs(ukfb_group* g, int64_t first, int64_t count, const double* gyro, const double* acc);
/* hot path from host arrays over the whole batch (z [total][3], Q [total][3][3]).  From 32 768 filters on, the host-array calls
 * of a group (these, ukfb_group_initialize, ukfb_group_get_state, ukfb_group_cycle_timestamps) run one host thread per shard for
 * the duration of the call, so that the uploads of all devices proceed at once over their own PCIe links. */
int ukfb_group_predict(ukfb_group* g, double dt);
int ukfb_group_update(ukfb_group* g, int meas_model, const double* z, const double* Q);
int ukfb_group_cycle(ukfb_group* g, double dt, int meas_model, const double* z, const double* Q);
/* hot path from device-resident inputs: arrays of one device pointer PER SHARD (index = shard, memory on that shard's
 * device, engine precision, sized for the shard's filters) -- the shapes of ukfb_cycle_dev / ukfb_cycle_multi_dev /
 * ukfb_pose_bind_acceleration_dev / ukfb_orient_bind_inputs_dev */
int ukfb_group_pose_bind_acceleration_dev(ukfb_group* g, const void* const* acc_mu_dev);
int ukfb_group_orient_bind_inputs_dev(ukfb_group* g, const void* const* gyro_dev, const void* const* acc_dev);
int ukfb_group_cycle_dev(ukfb_group* g, double dt, int meas_model, const void* const* z_dev, const void* const* Q_dev);
int ukfb_group_cycle_multi_dev(ukfb_group* g, int cycles, double dt, int meas_model, int slots, int first_slot,
                               const void* const* in_a_dev, const void* const* in_b_dev, const void* const* z_dev,
                               const void* const* Q_dev);
/* per-filter model ids resident on the devices (ukfb_cycle_dev with meas_model_dev), one pointer per shard */
int ukfb_group_cycle_mixed_dev(ukfb_group* g, double dt, const int32_t* const* meas_model_dev, const void* const* z_dev,
                               const void* const* Q_dev);
/* ukfb_cycle_timestamps over the whole batch: host arrays [total] in batch numbering */
int ukfb_group_cycle_timestamps(ukfb_group* g, const int64_t* ts_us, const int32_t* meas_model, const double* z, const double* Q);
/* ukfb_process_events over the whole batch: `filter` in batch numbering, any arrival order.  Events are routed to the shard
 * that owns their filter (stable: per filter the arrival order survives), the shards order and apply their events
 * concurrently (one host thread per shard for the duration of the call).  rounds = the launches of the shard that needed most;
 * statuses as ukfb_process_events leaves them (a filter without samples: 0). */
int ukfb_group_process_events(ukfb_group* g, int64_t n_events, const int64_t* filter, const int64_t* ts_us,
                              const int32_t* meas_model, const double* z, const double* Q, uint32_t* status_or, int64_t* rounds);
int ukfb_group_sync(ukfb_group* g);
/* HIP-event timing on every shard's stream; elapsed_ms_max = the slowest shard, elapsed_ms_per_shard [shards] may be NULL */
int ukfb_group_timer_begin(ukfb_group* g);
int ukfb_group_timer_end(ukfb_group* g, float* elapsed_ms_max, float* elapsed_ms_per_shard);
/* Result gather: out_dev[shard] -- memory on that shard's device, engine precision, [total_filters][S] -- receives the mean
 * states of ALL filters in batch order on every device: ncclAllGather over one communicator per device (ncclCommInitAll at
 * the first call; RCCL is loaded at run time, librccl.so.1).  Stream-ordered after the launches enqueued so far; complete
 * after ukfb_group_sync.  Gather at the end of a run or every K cycles, not per cycle: at 131 072 Pose filters per device
 * the means are 6.8 MB (fp32) per shard, about the duration of one cycle over xGMI.  A group whose shards SHARE a device
 * (where RCCL has no rank to give them; e.g. a rehearsal of N shards on one GPU) exchanges by peer copies between the shards'
 * streams instead; staging and the ragged compaction are the same code either way.  ukfb_group_last_gather_exchange tells
 * which exchange the last gather used: 1 = RCCL all-gather, 2 = peer copies, 0 = no gather yet, -1 = NULL group. */
int ukfb_group_gather_means(ukfb_group* g, void* const* out_dev);
int ukfb_group_last_gather_exchange(const ukfb_group* g);

/* ---- measurement of the engine itself ---------------------------------------------------- */
/* name, dynamic LDS bytes per workgroup, filters per workgroup and grid size of the kernel the
 * most recent predict/update/cycle call launched (for profiles/ and bench.py) */
int ukfb_last_launch_info(const ukfb_engine* e, char* kernel_name, int name_capacity, int* lds_bytes,
                          int* filters_per_workgroup, int64_t* grid);
/* the filter list of the most recent launch that grouped its filters by update class (ukfb_cycle_dev with per-filter
 * model ids, ukfb_config.bucket_models): *items = entries the launch covered, the first min(capacity, *items) of them
 * copied to list -- filter indices, class by class (sigma-point updates first, then the linear selections, then the
 * filters without a sample), every class starting at a multiple of 4, -1 = padding.  UKFB_ERR_INVALID_ARG when no
 * launch of the engine has been grouped. */
int ukfb_last_model_groups(ukfb_engine* e, int32_t* list, int64_t capacity, int64_t* items);
/* HIP-event timing on the engine's stream: begin/end bracket a region, elapsed in ms */
int ukfb_timer_begin(ukfb_engine* e);
int ukfb_timer_end(ukfb_engine* e, float* elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* UKF_BATCH_H */
