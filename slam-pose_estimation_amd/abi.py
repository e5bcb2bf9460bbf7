"""The binding's statement of the C ABI of include/ukf_batch.h, and nothing else: its constants, its structures and, in
SIGNATURES, the result and argument types of every entry point.

tests/test_binding_signatures.py reads the header and compares it with this file type by type: a prototype or a struct
member that changes there needs its line here, or the CPU suite fails.
"""
from __future__ import annotations

import ctypes as C

MODEL_POSE, MODEL_ORIENT = 0, 1
F64, F32 = 0, 1

MEAS_NONE = -1
MEAS_POS3, MEAS_POS_XY, MEAS_POS_Z, MEAS_ORIENT_SO3, MEAS_VEL3 = 0, 1, 2, 3, 4
MEAS_VEL_XY, MEAS_VEL_Z, MEAS_XVEL_YAWVEL, MEAS_ANGVEL3, MEAS_ORIENT_BODYVEL3 = 5, 6, 7, 8, 9

ST_OK = 0
ST_SKIPPED_FIRST_TS = 1 << 0
ST_SKIPPED_SMALL_DT = 1 << 1
ST_ERR_NEG_DT = 1 << 2
ST_ERR_DT_TOO_LARGE = 1 << 3
ST_ERR_NONFINITE_MEAS = 1 << 4
ST_ERR_CHOLESKY = 1 << 5
ST_WARN_MEAN_NOCONV = 1 << 6
ST_UNINITIALISED = 1 << 7
ST_INACTIVE = 1 << 8
ST_REJECTED_GATE = 1 << 9
ST_ERR_WEIGHTS = 1 << 10   # filter banks: the weights of a track are not a distribution
ST_REPAIRED = 1 << 11      # covariance conditioning: the covariance or the quaternion was repaired

BODY_STATE_SCALARS = 49

# state blocks of ukfb_update_state_dev, one bit each, in host-layout order
BLOCK_POSE_POSITION, BLOCK_POSE_ORIENTATION, BLOCK_POSE_VELOCITY, BLOCK_POSE_ANGULAR_VELOCITY = 1, 2, 4, 8
BLOCK_POSE_ALL = 15
BLOCK_ORIENT_ORIENTATION, BLOCK_ORIENT_VELOCITY, BLOCK_ORIENT_BIAS_GYRO, BLOCK_ORIENT_BIAS_ACC, BLOCK_ORIENT_GRAVITY = 1, 2, 4, 8, 16
BLOCK_ORIENT_ALL = 31

# models of ukfb_update_sensor_dev: 0 ... 4 the Pose engine's, 5 ... 7 the OrientationState engine's
SENSOR_NONE = -1
SENSOR_POSE_POSITION, SENSOR_POSE_RANGE, SENSOR_POSE_POINT, SENSOR_POSE_VELOCITY, SENSOR_POSE_NAV_VELOCITY = 0, 1, 2, 3, 4
SENSOR_ORIENT_VELOCITY, SENSOR_ORIENT_NAV_VECTOR, SENSOR_ORIENT_SPECIFIC_FORCE = 5, 6, 7
SENSOR_MOUNT_IDENTITY = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)   # r = 0, qs = (0, 0, 0, 1)

# models of ukfb_update_bearing_dev: 0, 1 the Pose engine's, 2 the OrientationState engine's
BEARING_NONE = -1
BEARING_POSE_POINT, BEARING_POSE_NAV_DIRECTION, BEARING_ORIENT_NAV_DIRECTION = 0, 1, 2

# most candidates per filter of ukfb_associate_sensor_dev (UKFB_ASSOCIATE_MAX_CANDIDATES)
ASSOCIATE_MAX_CANDIDATES = 32

# largest measurement dimension of ukfb_update_sampled_dev (UKFB_SAMPLED_MAX_M)
SAMPLED_MAX_M = 6


class Config(C.Structure):
    _fields_ = [("mean_tol", C.c_double), ("mean_max_iter", C.c_int32), ("gate_chi2", C.c_double),
                ("min_time_delta", C.c_double), ("max_time_delta", C.c_double), ("lanes_per_filter", C.c_int32),
                ("bucket_models", C.c_int32), ("split_streams", C.c_int32), ("wide_arithmetic", C.c_int32),
                ("full_update_check", C.c_int32)]


class InnovationOut(C.Structure):
    """ukfb_innovation_out: device pointers in engine precision, any may be NULL"""
    _fields_ = [("z_pred", C.c_void_p), ("S", C.c_void_p), ("innov", C.c_void_p), ("maha", C.c_void_p),
                ("loglik", C.c_void_p), ("best", C.c_void_p), ("status", C.c_void_p)]


class StateMeasOut(C.Structure):
    """ukfb_state_meas_out: device pointers in engine precision (status uint32), any may be NULL"""
    _fields_ = [("maha", C.c_void_p), ("loglik", C.c_void_p), ("status", C.c_void_p)]


class SensorIn(C.Structure):
    """ukfb_sensor_in: device pointers in engine precision (model_dev int32); the *_uniform values are host doubles"""
    _fields_ = [("model_dev", C.c_void_p), ("z_dev", C.c_void_p), ("Q_dev", C.c_void_p), ("q_is_uniform", C.c_int),
                ("mount_dev", C.c_void_p), ("mount_uniform", C.c_double * 7), ("point_dev", C.c_void_p),
                ("point_uniform", C.c_double * 3)]


class SensorOut(C.Structure):
    """ukfb_sensor_out: device pointers in engine precision (status uint32), any may be NULL"""
    _fields_ = [("z_pred", C.c_void_p), ("S", C.c_void_p), ("innov", C.c_void_p), ("maha", C.c_void_p),
                ("loglik", C.c_void_p), ("status", C.c_void_p)]


class AssociateIn(C.Structure):
    """ukfb_associate_in: ukfb_sensor_in with `candidates` slots of z ([candidates, capacity, 3]) and, with
    point_per_candidate, of the point"""
    _fields_ = [("model_dev", C.c_void_p), ("candidates", C.c_int), ("z_dev", C.c_void_p), ("Q_dev", C.c_void_p),
                ("q_is_uniform", C.c_int), ("mount_dev", C.c_void_p), ("mount_uniform", C.c_double * 7), ("point_dev", C.c_void_p),
                ("point_uniform", C.c_double * 3), ("point_per_candidate", C.c_int)]


class AssociateOut(C.Structure):
    """ukfb_associate_out: device pointers in engine precision (best, n_gated int32, status uint32), any may be NULL"""
    _fields_ = [("z_pred", C.c_void_p), ("S", C.c_void_p), ("innov", C.c_void_p), ("maha", C.c_void_p),
                ("loglik", C.c_void_p), ("best", C.c_void_p), ("n_gated", C.c_void_p), ("status", C.c_void_p)]


class SampledIn(C.Structure):
    """ukfb_sampled_in: the samples Z [capacity, 2 D + 1, m], z [capacity, m], Q [capacity, m, m] (or one m x m) as device
    pointers in engine precision; active_dev uint8 [capacity] or NULL"""
    _fields_ = [("m", C.c_int), ("Z_dev", C.c_void_p), ("z_dev", C.c_void_p), ("Q_dev", C.c_void_p), ("q_is_uniform", C.c_int),
                ("active_dev", C.c_void_p)]


class SampledOut(C.Structure):
    """ukfb_sampled_out: device pointers in engine precision (status uint32), any may be NULL"""
    _fields_ = [("z_pred", C.c_void_p), ("S", C.c_void_p), ("innov", C.c_void_p), ("maha", C.c_void_p),
                ("loglik", C.c_void_p), ("status", C.c_void_p)]


class PredictSampledIn(C.Structure):
    """ukfb_predict_sampled_in: the propagated points XX [capacity, 2 D + 1, S], R [capacity, D, D] (or one D x D) as device
    pointers in engine precision; active_dev uint8 [capacity] or NULL"""
    _fields_ = [("XX_dev", C.c_void_p), ("R_dev", C.c_void_p), ("r_is_uniform", C.c_int), ("active_dev", C.c_void_p)]


class PredictSampledOut(C.Structure):
    """ukfb_predict_sampled_out: device pointers in engine precision (status uint32), any may be NULL"""
    _fields_ = [("mu", C.c_void_p), ("cov_packed", C.c_void_p), ("status", C.c_void_p)]


class ConditionIn(C.Structure):
    """ukfb_condition_in: the variance floor [D] as a device pointer in engine precision, the correlation-eigenvalue floor (a host
    double), select_dev uint8 [capacity] or NULL, the renormalisation flag"""
    _fields_ = [("var_floor_dev", C.c_void_p), ("eig_floor", C.c_double), ("select_dev", C.c_void_p), ("renormalize_quaternion", C.c_int)]


class ConditionOut(C.Structure):
    """ukfb_condition_out: device pointers in engine precision (status uint32), any may be NULL"""
    _fields_ = [("eig_min", C.c_void_p), ("eig_max", C.c_void_p), ("mu", C.c_void_p), ("cov_packed", C.c_void_p), ("status", C.c_void_p)]


class DelayedIn(C.Structure):
    """ukfb_delayed_in: the window (dt a HOST array), the lags, the models and the sample; device pointers in engine precision"""
    _fields_ = [("steps", C.c_int), ("dt", C.POINTER(C.c_double)), ("slots", C.c_int), ("first_slot", C.c_int),
                ("mu_hist_dev", C.c_void_p), ("cov_hist_dev", C.c_void_p), ("in_a_dev", C.c_void_p), ("in_b_dev", C.c_void_p),
                ("lag_uniform", C.c_int), ("lag_dev", C.c_void_p), ("meas_model_uniform", C.c_int), ("meas_model_dev", C.c_void_p),
                ("z_dev", C.c_void_p), ("Q_dev", C.c_void_p), ("q_is_uniform", C.c_int)]


class DelayedOut(C.Structure):
    """ukfb_delayed_out: device pointers in engine precision (status uint32), any may be NULL"""
    _fields_ = [("z_pred", C.c_void_p), ("S", C.c_void_p), ("innov", C.c_void_p), ("maha", C.c_void_p), ("loglik", C.c_void_p),
                ("status", C.c_void_p), ("mu_out", C.c_void_p), ("cov_out", C.c_void_p)]


class FilterRecords(C.Structure):
    """ukfb_filter_records: device pointers, n records in item order, scalars in engine precision; any may be NULL (scatter needs
    mu and cov_packed)"""
    _fields_ = [("mu", C.c_void_p), ("cov_packed", C.c_void_p), ("last_ts_us", C.c_void_p), ("initialised", C.c_void_p),
                ("in_a", C.c_void_p), ("in_b", C.c_void_p), ("noise", C.c_void_p), ("status", C.c_void_p)]


# Scalars by exact width and signedness; a typed pointer (host or device array) by its element; ukfb_engine*, ukfb_group* and
# void* (_h) as addresses; handle and device-pointer out-parameters and the per-shard pointer arrays (_ph) as arrays of addresses.
_i, _i64, _u32, _d, _str, _h, _P = C.c_int, C.c_int64, C.c_uint32, C.c_double, C.c_char_p, C.c_void_p, C.POINTER
_pd, _pf, _pi, _pi32, _pi64, _pu8, _pu32, _ph = (_P(t) for t in (C.c_double, C.c_float, C.c_int, C.c_int32, C.c_int64, C.c_uint8,
                                                               C.c_uint32, C.c_void_p))

# entry point -> (restype, argtypes), in the header's order
SIGNATURES = {
    "ukfb_default_config": (_i, (_P(Config),)),
    "ukfb_layout_supported": (_i, (_i, _i)),
    "ukfb_create": (_i, (_ph, _i, _i, _i64, _i, _h)),
    "ukfb_create_on_stream": (_i, (_ph, _i, _i, _i64, _i, _h)),
    "ukfb_destroy": (_i, (_h,)),
    "ukfb_last_error": (_str, ()),
    "ukfb_set_config": (_i, (_h, _P(Config))),
    "ukfb_get_config": (_i, (_h, _P(Config))),
    "ukfb_sync": (_i, (_h,)),
    "ukfb_describe": (_i, (_h, _pi, _pi, _pi64, _pi, _pi, _pi)),
    "ukfb_initialize": (_i, (_h, _i64, _i64, _pd, _pd)),
    "ukfb_get_state": (_i, (_h, _i64, _i64, _pd, _pd, _pu8)),
    "ukfb_get_status": (_i, (_h, _i64, _i64, _pu32)),
    "ukfb_get_status_summary": (_i, (_h, _pu32)),
    "ukfb_set_last_measurement_time": (_i, (_h, _i64, _i64, _pi64)),
    "ukfb_get_last_measurement_time": (_i, (_h, _i64, _i64, _pi64)),
    "ukfb_device_views": (_i, (_h, _ph, _ph, _ph)),
    "ukfb_set_process_noise": (_i, (_h, _pd)),
    "ukfb_set_process_noise_per_filter": (_i, (_h, _i64, _i64, _pd)),
    "ukfb_get_process_noise": (_i, (_h, _i64, _pd)),
    "ukfb_pose_set_acceleration": (_i, (_h, _i64, _i64, _pd, _pd)),
    "ukfb_pose_bind_acceleration_dev": (_i, (_h, _h)),
    "ukfb_orient_set_params": (_i, (_h, _d, _d, _pd)),
    "ukfb_orient_set_inputs": (_i, (_h, _i64, _i64, _pd, _pd)),
    "ukfb_orient_bind_inputs_dev": (_i, (_h, _h, _h)),
    "ukfb_orient_get_rotation_rate": (_i, (_h, _i64, _i64, _pd)),
    "ukfb_pose_export_body_states": (_i, (_h, _i64, _i64, _pd)),
    "ukfb_pose_import_body_states": (_i, (_h, _i64, _i64, _pd)),
    "ukfb_predict": (_i, (_h, _d)),
    "ukfb_predict_dt": (_i, (_h, _pd)),
    "ukfb_predict_timestamps": (_i, (_h, _pi64)),
    "ukfb_predict_dt_dev": (_i, (_h, _pd)),
    "ukfb_predict_timestamps_dev": (_i, (_h, _pi64)),
    "ukfb_update": (_i, (_h, _i, _pd, _pd, _pu8)),
    "ukfb_update_mixed": (_i, (_h, _pi32, _pd, _pd)),
    "ukfb_update_dev": (_i, (_h, _i, _pi32, _h, _h)),
    "ukfb_cycle": (_i, (_h, _d, _i, _pd, _pd)),
    "ukfb_cycle_dev": (_i, (_h, _d, _i, _pi32, _h, _h)),
    "ukfb_update_uniform_q": (_i, (_h, _i, _pd, _pd, _pu8)),
    "ukfb_cycle_uniform_q": (_i, (_h, _d, _i, _pd, _pd)),
    "ukfb_cycle_uniform_q_dev": (_i, (_h, _d, _i, _h, _h)),
    "ukfb_cycle_multi_dev": (_i, (_h, _i, _d, _i, _i, _i, _h, _h, _h, _h)),
    "ukfb_cycle_multi_mixed_dev": (_i, (_h, _i, _d, _i, _i, _h, _h, _pi32, _h, _h)),
    "ukfb_cycle_schedule_dev": (_i, (_h, _i, _pd, _pi32, _i, _i, _h, _h, _h, _h)),
    "ukfb_cycle_multi": (_i, (_h, _i, _d, _i, _pd, _pd, _pd, _pd)),
    "ukfb_cycle_timestamps": (_i, (_h, _pi64, _pi32, _pd, _pd)),
    "ukfb_cycle_timestamps_dev": (_i, (_h, _pi64, _pi32, _h, _h)),
    "ukfb_process_events": (_i, (_h, _i64, _pi64, _pi64, _pi32, _pd, _pd, _pu32, _pi64)),
    "ukfb_process_events_dev": (_i, (_h, _i64, _pi64, _pi64, _pi32, _h, _h, _pu32, _pi64)),
    # innovation statistics / measurement association (read-only)
    "ukfb_innovation_dev": (_i, (_h, _i, _pi32, _i, _h, _h, _i, _P(InnovationOut))),
    "ukfb_select_candidates_dev": (_i, (_h, _i, _pi32, _i, _pi32, _h, _h, _pi32)),
    "ukfb_innovation": (_i, (_h, _i, _i, _pd, _pd, _pd, _pd, _pd, _pd, _pd, _pi32, _pu32)),
    # filter banks: IMM mixing, weights, mixture moments
    "ukfb_bank_weights_dev": (_i, (_h, _i, _h, _h, _h, _h, _pu32)),
    "ukfb_bank_combine_dev": (_i, (_h, _i, _h, _h, _h, _pu32)),
    "ukfb_bank_mix_dev": (_i, (_h, _i, _h, _pd, _h, _pu32)),
    "ukfb_bank_combine": (_i, (_h, _i, _pd, _pd, _pd, _pu32)),
    "ukfb_bank_mix": (_i, (_h, _i, _pd, _pd, _pd, _pu32)),
    # fixed-interval smoothing: history rings and the RTS backward pass (read-only)
    "ukfb_history_push_dev": (_i, (_h, _i, _i, _h, _h)),
    "ukfb_smooth_dev": (_i, (_h, _i, _pd, _i, _i, _h, _h, _h, _h, _h, _h, _pu32)),
    "ukfb_smooth": (_i, (_h, _i, _pd, _pd, _pd, _pd, _pd, _pu32)),
    # late samples: the delayed-measurement update through the state history
    "ukfb_update_delayed_dev": (_i, (_h, _P(DelayedIn), _i, _P(DelayedOut))),
    "ukfb_update_delayed": (_i, (_h, _i, _pd, _pd, _pd, _pd, _pd, _i, _pi32, _i, _pi32, _pd, _pd, _i, _pd, _pd, _pd, _pd, _pd, _pu32, _pd, _pd)),
    "ukfb_delayed_lag_dev": (_i, (_h, _i, _pi64, _pi64, _pi32)),
    # forecast: multi-step prediction from a start record into a ring of the history's format (read-only)
    "ukfb_forecast_dev": (_i, (_h, _i, _pd, _pi64, _i, _i, _h, _h, _h, _h, _h, _h, _pu32)),
    "ukfb_forecast": (_i, (_h, _i, _pd, _pi64, _pd, _pd, _pd, _pd, _pd, _pd, _pu32)),
    # filter lifecycle: whole per-filter records gathered and scattered on the device, retirement, in-place compaction
    "ukfb_gather_filters_dev": (_i, (_h, _i64, _pi32, _P(FilterRecords))),
    "ukfb_scatter_filters_dev": (_i, (_h, _i64, _pi32, _P(FilterRecords))),
    "ukfb_retire_dev": (_i, (_h, _pu8)),
    "ukfb_compact_dev": (_i, (_h, _i, _pi32, _pi32, _pi64)),
    "ukfb_gather_filters": (_i, (_h, _i64, _pi32, _pd, _pd, _pi64, _pu8)),
    "ukfb_scatter_filters": (_i, (_h, _i64, _pi32, _pd, _pd, _pi64, _pu8, _pu32)),
    "ukfb_compact": (_i, (_h, _i, _pi32, _pi32, _pi64)),
    # joint state-block measurements: update / fuse with full covariance, covariance intersection, track-to-track distance
    "ukfb_update_state_dev": (_i, (_h, _u32, _pi32, _h, _h, _d, _d, _i, _P(StateMeasOut))),
    "ukfb_update_state": (_i, (_h, _u32, _pi32, _pd, _pd, _d, _d, _i, _pd, _pd, _pu32)),
    "ukfb_pose_update_body_states": (_i, (_h, _u32, _pd, _pu8)),
    # sensor-frame measurements: lever arms, ranges, landmark fixes, nav-frame vectors
    "ukfb_update_sensor_dev": (_i, (_h, _i, _P(SensorIn), _i, _P(SensorOut))),
    "ukfb_update_sensor": (_i, (_h, _i, _pi32, _pd, _pd, _pd, _pd, _pd, _pd, _i, _pd, _pd, _pd, _pd, _pd, _pu32)),
    # bearing measurements: directions on the sphere S^2
    "ukfb_update_bearing_dev": (_i, (_h, _i, _P(SensorIn), _i, _P(SensorOut))),
    "ukfb_update_bearing": (_i, (_h, _i, _pi32, _pd, _pd, _pd, _pd, _pd, _pd, _i, _pd, _pd, _pd, _pd, _pd, _pu32)),
    # sensor-frame association: K candidates per filter scored in one launch, the nearest inside the gate committed
    "ukfb_associate_sensor_dev": (_i, (_h, _i, _P(AssociateIn), _i, _P(AssociateOut))),
    "ukfb_associate_sensor": (_i, (_h, _i, _pi32, _i, _pd, _pd, _pd, _pd, _pd, _pd, _i, _i, _pd, _pd, _pd, _pd, _pd, _pi32, _pi32, _pu32)),
    # user-defined measurement models: sigma-point export, the update finished from the caller's samples
    "ukfb_sigma_points_dev": (_i, (_h, _h, _h, _pu32)),
    "ukfb_update_sampled_dev": (_i, (_h, _P(SampledIn), _i, _P(SampledOut))),
    "ukfb_sigma_points": (_i, (_h, _pd, _pd, _pu32)),
    "ukfb_update_sampled": (_i, (_h, _i, _pd, _pd, _pd, _i, _pu8, _i, _pd, _pd, _pd, _pd, _pd, _pu32)),
    # user-defined process models: the prediction finished from the caller's propagated sigma points
    "ukfb_predict_sampled_dev": (_i, (_h, _P(PredictSampledIn), _i, _P(PredictSampledOut))),
    "ukfb_predict_sampled": (_i, (_h, _pd, _pd, _i, _pu8, _i, _pd, _pd, _pu32)),
    # covariance conditioning: eigenvalue repair of failed filters, quaternion renormalisation
    "ukfb_condition_dev": (_i, (_h, _P(ConditionIn), _i, _P(ConditionOut))),
    "ukfb_condition": (_i, (_h, _pd, _d, _pu8, _i, _i, _pd, _pd, _pd, _pd, _pu32)),
    # device groups (one process, several GPUs)
    "ukfb_group_shard_range": (_i, (_i64, _i, _i, _pi64, _pi64)),
    "ukfb_group_create": (_i, (_ph, _i, _i, _i64, _pi, _i)),
    "ukfb_group_destroy": (_i, (_h,)),
    "ukfb_group_size": (_i, (_h,)),
    "ukfb_group_shard": (_i, (_h, _i, _ph, _pi, _pi64, _pi64)),
    "ukfb_group_set_config": (_i, (_h, _P(Config))),
    "ukfb_group_initialize": (_i, (_h, _i64, _i64, _pd, _pd)),
    "ukfb_group_get_state": (_i, (_h, _i64, _i64, _pd, _pd, _pu8)),
    "ukfb_group_get_status": (_i, (_h, _i64, _i64, _pu32)),
    "ukfb_group_get_status_summary": (_i, (_h, _pu32)),
    "ukfb_group_set_process_noise": (_i, (_h, _pd)),
    "ukfb_group_pose_set_acceleration": (_i, (_h, _i64, _i64, _pd, _pd)),
    "ukfb_group_orient_set_params": (_i, (_h, _d, _d, _pd)),
    "ukfb_group_orient_set_inputs": (_i, (_h, _i64, _i64, _pd, _pd)),
    "ukfb_group_predict": (_i, (_h, _d)),
    "ukfb_group_update": (_i, (_h, _i, _pd, _pd)),
    "ukfb_group_cycle": (_i, (_h, _d, _i, _pd, _pd)),
    "ukfb_group_pose_bind_acceleration_dev": (_i, (_h, _ph)),
    "ukfb_group_orient_bind_inputs_dev": (_i, (_h, _ph, _ph)),
    "ukfb_group_cycle_dev": (_i, (_h, _d, _i, _ph, _ph)),
    "ukfb_group_cycle_multi_dev": (_i, (_h, _i, _d, _i, _i, _i, _ph, _ph, _ph, _ph)),
    "ukfb_group_cycle_mixed_dev": (_i, (_h, _d, _ph, _ph, _ph)),
    "ukfb_group_cycle_timestamps": (_i, (_h, _pi64, _pi32, _pd, _pd)),
    "ukfb_group_process_events": (_i, (_h, _i64, _pi64, _pi64, _pi32, _pd, _pd, _pu32, _pi64)),
    "ukfb_group_sync": (_i, (_h,)),
    "ukfb_group_timer_begin": (_i, (_h,)),
    "ukfb_group_timer_end": (_i, (_h, _pf, _pf)),
    "ukfb_group_gather_means": (_i, (_h, _ph)),
    "ukfb_group_last_gather_exchange": (_i, (_h,)),
    # measurement of the engine
    "ukfb_last_launch_info": (_i, (_h, _str, _i, _pi, _pi, _pi64)),
    "ukfb_last_model_groups": (_i, (_h, _pi32, _i64, _pi64)),
    "ukfb_timer_begin": (_i, (_h,)),
    "ukfb_timer_end": (_i, (_h, _pf)),
}

# every symbol include/ukf_batch.h declares (tests check the library exports all of them)
EXPORTS = list(SIGNATURES)


def declare(lib):
    """Set restype and argtypes on every entry point of a loaded CDLL; a missing symbol raises AttributeError."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
