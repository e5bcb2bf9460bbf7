"""ctypes binding of the C-ABI in include/ukf_batch.h (lib/libukf_batch.so).

This is plumbing: every numeric operation happens in the HIP kernels behind the C-ABI.  There is no
CPU fallback -- if the shared library or a HIP device is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UKFB_LIB", os.path.join(_HERE, "lib", "libukf_batch.so"))  # UKFB_LIB: debug builds only

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

# every symbol include/ukf_batch.h declares (tests check the library exports all of them)
EXPORTS = [
    "ukfb_default_config", "ukfb_layout_supported", "ukfb_create", "ukfb_create_on_stream", "ukfb_destroy", "ukfb_last_error", "ukfb_set_config", "ukfb_get_config",
    "ukfb_sync", "ukfb_describe", "ukfb_initialize", "ukfb_get_state", "ukfb_get_status", "ukfb_get_status_summary",
    "ukfb_set_last_measurement_time", "ukfb_get_last_measurement_time", "ukfb_device_views",
    "ukfb_set_process_noise", "ukfb_set_process_noise_per_filter", "ukfb_get_process_noise",
    "ukfb_pose_set_acceleration", "ukfb_pose_bind_acceleration_dev", "ukfb_orient_set_params",
    "ukfb_orient_set_inputs", "ukfb_orient_bind_inputs_dev", "ukfb_orient_get_rotation_rate", "ukfb_predict",
    "ukfb_predict_dt", "ukfb_predict_timestamps", "ukfb_predict_dt_dev", "ukfb_predict_timestamps_dev",
    "ukfb_update", "ukfb_update_mixed", "ukfb_update_dev", "ukfb_cycle", "ukfb_cycle_dev", "ukfb_cycle_multi_dev", "ukfb_cycle_multi",
    "ukfb_cycle_schedule_dev", "ukfb_cycle_multi_mixed_dev", "ukfb_update_uniform_q", "ukfb_cycle_uniform_q",
    "ukfb_cycle_uniform_q_dev",
    "ukfb_last_launch_info",
    "ukfb_last_model_groups",
    "ukfb_timer_begin", "ukfb_timer_end", "ukfb_pose_export_body_states", "ukfb_pose_import_body_states",
    "ukfb_cycle_timestamps", "ukfb_cycle_timestamps_dev", "ukfb_process_events", "ukfb_process_events_dev",
    # innovation statistics / measurement association (read-only)
    "ukfb_innovation_dev", "ukfb_select_candidates_dev", "ukfb_innovation",
    # filter banks: IMM mixing, weights, mixture moments
    "ukfb_bank_weights_dev", "ukfb_bank_combine_dev", "ukfb_bank_mix_dev", "ukfb_bank_combine", "ukfb_bank_mix",
    # fixed-interval smoothing: history rings and the RTS backward pass (read-only)
    "ukfb_history_push_dev", "ukfb_smooth_dev", "ukfb_smooth",
    # forecast: multi-step prediction from a start record into a ring of the history's format (read-only)
    "ukfb_forecast_dev", "ukfb_forecast",
    # filter lifecycle: whole per-filter records gathered and scattered on the device, retirement, in-place compaction
    "ukfb_gather_filters_dev", "ukfb_scatter_filters_dev", "ukfb_retire_dev", "ukfb_compact_dev",
    "ukfb_gather_filters", "ukfb_scatter_filters", "ukfb_compact",
    # joint state-block measurements: update / fuse with full covariance, covariance intersection, track-to-track distance
    "ukfb_update_state_dev", "ukfb_update_state", "ukfb_pose_update_body_states",
    # sensor-frame measurements: lever arms, ranges, landmark fixes, nav-frame vectors
    "ukfb_update_sensor_dev", "ukfb_update_sensor",
    # bearing measurements: directions on the sphere S^2
    "ukfb_update_bearing_dev", "ukfb_update_bearing",
    # sensor-frame association: K candidates per filter scored in one launch, the nearest inside the gate committed
    "ukfb_associate_sensor_dev", "ukfb_associate_sensor",
    # user-defined measurement models: sigma-point export, the update finished from the caller's samples
    "ukfb_sigma_points_dev", "ukfb_update_sampled_dev", "ukfb_sigma_points", "ukfb_update_sampled",
    # user-defined process models: the prediction finished from the caller's propagated sigma points
    "ukfb_predict_sampled_dev", "ukfb_predict_sampled",
    # late samples: the delayed-measurement update through the state history
    "ukfb_update_delayed_dev", "ukfb_update_delayed", "ukfb_delayed_lag_dev",
    # covariance conditioning: eigenvalue repair of failed filters, quaternion renormalisation
    "ukfb_condition_dev", "ukfb_condition",
    # device groups (one process, several GPUs)
    "ukfb_group_shard_range", "ukfb_group_create", "ukfb_group_destroy", "ukfb_group_size", "ukfb_group_shard",
    "ukfb_group_set_config", "ukfb_group_initialize", "ukfb_group_get_state", "ukfb_group_get_status",
    "ukfb_group_get_status_summary", "ukfb_group_set_process_noise", "ukfb_group_pose_set_acceleration",
    "ukfb_group_orient_set_params", "ukfb_group_orient_set_inputs", "ukfb_group_predict", "ukfb_group_update",
    "ukfb_group_cycle", "ukfb_group_pose_bind_acceleration_dev", "ukfb_group_orient_bind_inputs_dev",
    "ukfb_group_cycle_dev", "ukfb_group_cycle_multi_dev", "ukfb_group_cycle_mixed_dev", "ukfb_group_cycle_timestamps",
    "ukfb_group_process_events", "ukfb_group_sync", "ukfb_group_timer_begin",
    "ukfb_group_timer_end", "ukfb_group_gather_means", "ukfb_group_last_gather_exchange",
]
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


class UkfbError(RuntimeError):
    pass


_lib = None


def load_library():
    """Load libukf_batch.so; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise UkfbError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                            f"(make -C slam-pose_estimation_amd/csrc); there is no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        lib.ukfb_last_error.restype = C.c_char_p
        _lib = lib
    return _lib


def _chk(rc: int, what: str):
    if rc != 0:
        msg = load_library().ukfb_last_error()
        raise UkfbError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _devptr(x):
    """Accept an int address, a torch tensor (data_ptr) or None."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


def _ptr(x):
    """The address behind _devptr as a plain int, or None: what a pointer field of a ctypes Structure takes."""
    return None if x is None else _devptr(x).value


def _typed_pointer(ctype):
    return lambda a: a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


# the ctypes pointer of a NumPy array of that element type, None for None (as _pd for doubles)
_pi32, _pu32, _pu8, _pi64 = (_typed_pointer(t) for t in (C.c_int32, C.c_uint32, C.c_uint8, C.c_int64))


def _int_or_i32(x, n):
    """An argument that is one int for the batch or an int32 array [n] -> (the int or 0, the array or None)."""
    if np.isscalar(x):
        return int(x), None
    return 0, np.ascontiguousarray(x, dtype=np.int32).reshape(n)


def _per_or_uniform(a, n, width):
    """A host value [width] for the batch or an array [n, width] per filter (mount, point) -> (per-filter, uniform), one None."""
    a = _f64(a)
    return (a.reshape(n, width), None) if a.ndim == 2 else (None, a.reshape(width))


def _torch_current_stream(device: int):
    """hipStream_t of torch's current stream on `device` (0 = the default stream), or None when torch is not in use."""
    import sys
    torch = sys.modules.get("torch")
    if torch is None:
        return None
    try:
        if not torch.cuda.is_available():
            return None
        return int(torch.cuda.current_stream(device).cuda_stream)
    except Exception:
        return None


def layout_supported(precision: int, lanes_per_filter: int) -> bool:
    return bool(load_library().ukfb_layout_supported(C.c_int(precision), C.c_int(lanes_per_filter)))


class BatchUKF:
    """A batch of independent UKFs resident on one MI355X (opaque ukfb_engine handle)."""

    def __init__(self, model: int, precision: int, capacity: int, device: int = 0, stream=None,
                 lanes_per_filter: int = 0, **cfg):
        """stream:
          "private"  an engine-owned non-blocking stream, what ukfb_create gives a C caller (bench.py: nothing else shares
                     the timed stream; small batches run as split launches on two internal streams, ukfb_config.split_streams);
          "torch"    torch's CURRENT stream on `device` (tensors the caller produces with torch and hands to the "_dev" entry
                     points are then ordered with the engine's launches without any synchronise); raises without torch / a GPU;
          an int     that hipStream_t;
          None       "torch" when torch is imported and sees a GPU, else "private" -- the convenient default of this binding;
                     `stream_kind` ("private" / "torch" / "given") tells which one an engine got."""
        self._lib = load_library()
        self._h = C.c_void_p()
        args = (C.byref(self._h), C.c_int(model), C.c_int(precision), C.c_int64(capacity), C.c_int(device))
        kind = "given"
        if stream is None or stream == "torch":
            ts = _torch_current_stream(device)
            if ts is None and stream == "torch":
                raise UkfbError('stream="torch" needs torch with a visible GPU')
            kind = "torch" if ts is not None else "private"
            stream = ts if ts is not None else "private"
        if stream == "private":
            self.stream_kind = "private"
            _chk(self._lib.ukfb_create(*args, None), "ukfb_create")
        else:
            self.stream_kind = kind
            _chk(self._lib.ukfb_create_on_stream(*args, C.c_void_p(int(stream)) if int(stream) else None), "ukfb_create_on_stream")
        self.model, self.precision, self.capacity, self.device = model, precision, int(capacity), device
        self.S = 13 if model == MODEL_POSE else 14
        self.D = 12 if model == MODEL_POSE else 13
        self.PK = self.D * (self.D + 1) // 2
        self.dtype = np.float64 if precision == F64 else np.float32
        if lanes_per_filter or cfg:
            self.configure(lanes_per_filter=lanes_per_filter, **cfg)

    # ---- lifetime / config
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ukfb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def config(self) -> Config:
        c = Config()
        _chk(self._lib.ukfb_get_config(self._h, C.byref(c)), "ukfb_get_config")
        return c

    def configure(self, **kw):
        c = self.config()
        for k, v in kw.items():
            if k == "lanes_per_filter" and not v:
                continue
            setattr(c, k, v)
        _chk(self._lib.ukfb_set_config(self._h, C.byref(c)), "ukfb_set_config")

    def sync(self):
        _chk(self._lib.ukfb_sync(self._h), "ukfb_sync")

    # ---- state
    def initialize(self, mu, cov, first: int = 0):
        mu = _f64(mu, (-1, self.S)); cov = _f64(cov, (-1, self.D, self.D))
        _chk(self._lib.ukfb_initialize(self._h, C.c_int64(first), C.c_int64(mu.shape[0]), _pd(mu), _pd(cov)),
             "ukfb_initialize")

    def state(self, first: int = 0, count: Optional[int] = None, with_cov: bool = True):
        count = self.capacity - first if count is None else count
        mu = np.empty((count, self.S))
        cov = np.empty((count, self.D, self.D)) if with_cov else None
        init = np.empty(count, dtype=np.uint8)
        _chk(self._lib.ukfb_get_state(self._h, C.c_int64(first), C.c_int64(count), _pd(mu), _pd(cov), _pu8(init)),
             "ukfb_get_state")
        return (mu, cov, init.astype(bool)) if with_cov else (mu, init.astype(bool))

    def status(self, first: int = 0, count: Optional[int] = None):
        count = self.capacity - first if count is None else count
        st = np.empty(count, dtype=np.uint32)
        _chk(self._lib.ukfb_get_status(self._h, C.c_int64(first), C.c_int64(count), _pu32(st)), "ukfb_get_status")
        return st

    def status_summary(self) -> int:
        v = C.c_uint32(0)
        _chk(self._lib.ukfb_get_status_summary(self._h, C.byref(v)), "ukfb_get_status_summary")
        return int(v.value)

    def set_last_measurement_time(self, t_us, first: int = 0):
        t = np.ascontiguousarray(t_us, dtype=np.int64)
        _chk(self._lib.ukfb_set_last_measurement_time(self._h, C.c_int64(first), C.c_int64(t.size), _pi64(t)), "set_last_time")

    def last_measurement_time(self, first: int = 0, count: Optional[int] = None):
        count = self.capacity - first if count is None else count
        t = np.empty(count, dtype=np.int64)
        _chk(self._lib.ukfb_get_last_measurement_time(self._h, C.c_int64(first), C.c_int64(count), _pi64(t)), "get_last_time")
        return t

    def device_views(self):
        mu, cov, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _chk(self._lib.ukfb_device_views(self._h, C.byref(mu), C.byref(cov), C.byref(st)), "ukfb_device_views")
        return mu.value, cov.value, st.value

    # ---- noise / inputs
    def set_process_noise(self, R, first: Optional[int] = None):
        R = _f64(R)
        if R.ndim == 2:
            _chk(self._lib.ukfb_set_process_noise(self._h, _pd(R)), "ukfb_set_process_noise")
        else:
            _chk(self._lib.ukfb_set_process_noise_per_filter(self._h, C.c_int64(first or 0), C.c_int64(R.shape[0]),
                                                             _pd(R)), "ukfb_set_process_noise_per_filter")

    def process_noise(self, filter_index: int = 0):
        R = np.empty((self.D, self.D))
        _chk(self._lib.ukfb_get_process_noise(self._h, C.c_int64(filter_index), _pd(R)), "ukfb_get_process_noise")
        return R

    def set_acceleration(self, acc_mu=None, acc_cov=None, first: int = 0):
        am = _f64(acc_mu, (-1, 3)) if acc_mu is not None else None
        ac = _f64(acc_cov, (3, 3)) if acc_cov is not None else None
        n = am.shape[0] if am is not None else 0
        _chk(self._lib.ukfb_pose_set_acceleration(self._h, C.c_int64(first), C.c_int64(n), _pd(am), _pd(ac)),
             "ukfb_pose_set_acceleration")

    def export_body_states(self, first: int = 0, count: Optional[int] = None):
        """BodyStateMeasurement::toRigidBodyState for a range of filters -> [count, 49] records."""
        count = self.capacity - first if count is None else count
        out = np.empty((count, BODY_STATE_SCALARS))
        _chk(self._lib.ukfb_pose_export_body_states(self._h, C.c_int64(first), C.c_int64(count), _pd(out)),
             "ukfb_pose_export_body_states")
        return out

    def import_body_states(self, records, first: int = 0):
        """BodyStateMeasurement::fromRigidBodyState + initializeFilter from [count, 49] records."""
        rec = _f64(records, (-1, BODY_STATE_SCALARS))
        _chk(self._lib.ukfb_pose_import_body_states(self._h, C.c_int64(first), C.c_int64(rec.shape[0]), _pd(rec)),
             "ukfb_pose_import_body_states")

    def bind_acceleration_dev(self, acc_dev):
        _chk(self._lib.ukfb_pose_bind_acceleration_dev(self._h, _devptr(acc_dev)), "ukfb_pose_bind_acceleration_dev")

    def set_orient_params(self, gyro_bias_tau: float, acc_bias_tau: float, earth_rotation):
        er = _f64(earth_rotation, (3,))
        _chk(self._lib.ukfb_orient_set_params(self._h, C.c_double(gyro_bias_tau), C.c_double(acc_bias_tau), _pd(er)),
             "ukfb_orient_set_params")

    def set_orient_inputs(self, gyro=None, acc=None, first: int = 0):
        g = _f64(gyro, (-1, 3)) if gyro is not None else None
        a = _f64(acc, (-1, 3)) if acc is not None else None
        n = g.shape[0] if g is not None else (a.shape[0] if a is not None else 0)
        _chk(self._lib.ukfb_orient_set_inputs(self._h, C.c_int64(first), C.c_int64(n), _pd(g), _pd(a)),
             "ukfb_orient_set_inputs")

    def bind_orient_inputs_dev(self, gyro_dev, acc_dev):
        _chk(self._lib.ukfb_orient_bind_inputs_dev(self._h, _devptr(gyro_dev), _devptr(acc_dev)),
             "ukfb_orient_bind_inputs_dev")

    def rotation_rate(self, first: int = 0, count: Optional[int] = None):
        count = self.capacity - first if count is None else count
        out = np.empty((count, 3))
        _chk(self._lib.ukfb_orient_get_rotation_rate(self._h, C.c_int64(first), C.c_int64(count), _pd(out)),
             "ukfb_orient_get_rotation_rate")
        return out

    # ---- predict
    def predict(self, dt):
        if np.isscalar(dt):
            _chk(self._lib.ukfb_predict(self._h, C.c_double(float(dt))), "ukfb_predict")
        else:
            d = _f64(dt, (self.capacity,))
            _chk(self._lib.ukfb_predict_dt(self._h, _pd(d)), "ukfb_predict_dt")

    def predict_timestamps(self, ts_us):
        t = np.ascontiguousarray(ts_us, dtype=np.int64).reshape(self.capacity)
        _chk(self._lib.ukfb_predict_timestamps(self._h, _pi64(t)), "ukfb_predict_timestamps")

    def predict_dt_dev(self, dt_dev):
        _chk(self._lib.ukfb_predict_dt_dev(self._h, _devptr(dt_dev)), "ukfb_predict_dt_dev")

    def predict_timestamps_dev(self, ts_dev):
        _chk(self._lib.ukfb_predict_timestamps_dev(self._h, _devptr(ts_dev)), "ukfb_predict_timestamps_dev")

    # ---- update
    def update(self, meas_model, z, Q, active=None):
        z = _f64(z, (self.capacity, 3)); Q = _f64(Q, (self.capacity, 3, 3))
        if np.isscalar(meas_model):
            act = np.ascontiguousarray(active, dtype=np.uint8) if active is not None else None
            _chk(self._lib.ukfb_update(self._h, C.c_int(int(meas_model)), _pd(z), _pd(Q), _pu8(act)), "ukfb_update")
        else:
            m = np.ascontiguousarray(meas_model, dtype=np.int32).reshape(self.capacity)
            _chk(self._lib.ukfb_update_mixed(self._h, _pi32(m), _pd(z), _pd(Q)), "ukfb_update_mixed")

    def update_dev(self, meas_model_uniform: int, z_dev, Q_dev, meas_model_dev=None):
        _chk(self._lib.ukfb_update_dev(self._h, C.c_int(meas_model_uniform), _devptr(meas_model_dev), _devptr(z_dev),
                                       _devptr(Q_dev)), "ukfb_update_dev")

    # ---- innovation statistics and association (read-only: the engine's state and status are not touched)
    def innovation_dev(self, meas_model_uniform: int, candidates: int, z_dev, Q_dev, q_is_uniform: bool = False,
                       meas_model_dev=None, z_pred=None, S=None, innov=None, maha=None, loglik=None, best=None, status=None):
        """z_dev [candidates][capacity][3], Q_dev [capacity][9] (or 9 scalars with q_is_uniform); the keyword outputs are
        device buffers in engine precision (best int32, status uint32), None = not wanted.  Stream-ordered."""
        out = InnovationOut(_ptr(z_pred), _ptr(S), _ptr(innov), _ptr(maha), _ptr(loglik), _ptr(best), _ptr(status))
        _chk(self._lib.ukfb_innovation_dev(self._h, C.c_int(meas_model_uniform), _devptr(meas_model_dev), C.c_int(candidates),
                                           _devptr(z_dev), _devptr(Q_dev), C.c_int(1 if q_is_uniform else 0), C.byref(out)),
             "ukfb_innovation_dev")

    def select_candidates_dev(self, candidates: int, best_dev, meas_model_uniform: int, z_dev, z_sel_dev, meas_model_sel_dev=None,
                              meas_model_dev=None):
        """z_sel[i] = z[best[i]][i], meas_model_sel[i] = -1 where best[i] < 0: update_dev(0, z_sel, Q, meas_model_sel) then
        applies the nearest gated candidate of every filter and leaves the others untouched."""
        _chk(self._lib.ukfb_select_candidates_dev(self._h, C.c_int(candidates), _devptr(best_dev), C.c_int(meas_model_uniform),
                                                  _devptr(meas_model_dev), _devptr(z_dev), _devptr(z_sel_dev),
                                                  _devptr(meas_model_sel_dev)), "ukfb_select_candidates_dev")

    def innovation(self, meas_model: int, z, Q):
        """Host arrays: z [candidates, capacity, 3] (or [capacity, 3] for one candidate), Q [capacity, 3, 3].  Returns a dict of
        NumPy arrays: z_pred [n, 4], S [n, 3, 3], innov [K, n, 3], maha [K, n], loglik [K, n], best [n], status [n]."""
        n = self.capacity
        z = _f64(z, (-1, n, 3)); Q = _f64(Q, (n, 3, 3))
        K = z.shape[0]
        o = {"z_pred": np.empty((n, 4)), "S": np.empty((n, 3, 3)), "innov": np.empty((K, n, 3)), "maha": np.empty((K, n)),
             "loglik": np.empty((K, n)), "best": np.empty(n, dtype=np.int32), "status": np.empty(n, dtype=np.uint32)}
        _chk(self._lib.ukfb_innovation(self._h, C.c_int(int(meas_model)), C.c_int(K), _pd(z), _pd(Q), _pd(o["z_pred"]),
                                       _pd(o["S"]), _pd(o["innov"]), _pd(o["maha"]), _pd(o["loglik"]), _pi32(o["best"]),
                                       _pu32(o["status"])), "ukfb_innovation")
        return o

    # ---- filter banks: capacity / M tracks of M hypotheses, track-major (hypothesis j of track t = filter t * M + j)
    def bank_weights_dev(self, hypotheses: int, logw_in, loglik, logw_out, w_out=None, status=None):
        """logw_out = logw_in + loglik - logsumexp over a track's hypotheses, w_out = exp(logw_out).  Torch tensors (or device
        addresses) of [capacity] in engine precision; logw_in None = uniform, loglik None = normalise only; status uint32 [T]."""
        _chk(self._lib.ukfb_bank_weights_dev(self._h, C.c_int(hypotheses), _devptr(logw_in), _devptr(loglik), _devptr(logw_out),
                                             _devptr(w_out), _devptr(status)), "ukfb_bank_weights_dev")

    def bank_combine_dev(self, hypotheses: int, w, mu_out, cov_packed_out=None, status=None):
        """Mixture moments of every track: w [capacity], mu_out [T, S], cov_packed_out [T, PK] (lower triangle).  Read-only."""
        _chk(self._lib.ukfb_bank_combine_dev(self._h, C.c_int(hypotheses), _devptr(w), _devptr(mu_out), _devptr(cov_packed_out),
                                             _devptr(status)), "ukfb_bank_combine_dev")

    def bank_mix_dev(self, hypotheses: int, w, transition, w_pred=None, status=None):
        """IMM interaction: every hypothesis replaced by the mixture of its track under the mixing weights; transition is a HOST
        [M, M] row-stochastic matrix, w a device tensor [capacity].  Returns (w_pred, status): the caller's buffers ([capacity]
        in engine precision, int32 [T]) where given -- the call then allocates nothing -- else torch tensors created here."""
        P = _f64(transition, (hypotheses, hypotheses))
        if w_pred is None or status is None:
            import torch
            if w_pred is None:
                w_pred = torch.empty_like(w)
            if status is None:
                status = torch.empty(self.capacity // max(int(hypotheses), 1), dtype=torch.int32, device=w.device)
        _chk(self._lib.ukfb_bank_mix_dev(self._h, C.c_int(hypotheses), _devptr(w), _pd(P), _devptr(w_pred), _devptr(status)),
             "ukfb_bank_mix_dev")
        return w_pred, status

    def bank_combine(self, hypotheses: int, w):
        """Host arrays: w [capacity] -> (mu [T, S], cov [T, D, D], status [T])"""
        w = _f64(w, (self.capacity,))
        T = self.capacity // max(int(hypotheses), 1)
        mu, cov, st = np.empty((T, self.S)), np.empty((T, self.D, self.D)), np.empty(T, dtype=np.uint32)
        _chk(self._lib.ukfb_bank_combine(self._h, C.c_int(hypotheses), _pd(w), _pd(mu), _pd(cov), _pu32(st)), "ukfb_bank_combine")
        return mu, cov, st

    def bank_mix(self, hypotheses: int, w, transition):
        """Host arrays: w [capacity], transition [M, M] -> (w_pred [capacity], status [T]); replaces mean and covariance"""
        w = _f64(w, (self.capacity,))
        P = _f64(transition, (hypotheses, hypotheses))
        T = self.capacity // max(int(hypotheses), 1)
        wp, st = np.empty(self.capacity), np.empty(T, dtype=np.uint32)
        _chk(self._lib.ukfb_bank_mix(self._h, C.c_int(hypotheses), _pd(w), _pd(P), _pd(wp), _pu32(st)), "ukfb_bank_mix")
        return wp, st

    # ---- fixed-interval smoothing: history rings [slots, capacity, S] / [slots, capacity, PK] in engine precision
    def history_push_dev(self, slots: int, slot: int, mu_hist, cov_hist):
        """Stream-ordered copy of the engine's current mean and packed covariance into slot `slot` of the caller's rings (torch
        tensors or device addresses); ordered behind every launch enqueued so far, split launches included.  No allocation."""
        _chk(self._lib.ukfb_history_push_dev(self._h, C.c_int(slots), C.c_int(slot), _devptr(mu_hist), _devptr(cov_hist)),
             "ukfb_history_push_dev")

    def smooth_dev(self, dt, slots: int, first_slot: int, mu_hist, cov_hist, mu_out=None, cov_out=None, status=None,
                   in_a_dev=None, in_b_dev=None):
        """RTS backward pass over the window of len(dt) + 1 steps that starts at slot first_slot (step c in slot (first_slot + c)
        % slots); dt[c] (host) is the time step of the prediction c -> c + 1.  mu_out / cov_out: rings like the history, None =
        in place (pass cov_out=False for no covariance output); status uint32 / int32 [capacity] or None; in_a_dev / in_b_dev:
        input rings [slots, capacity, 3] or None (the latched inputs).  Caller-supplied buffers: nothing is allocated.
        Read-only on the engine.  Returns (mu_out, cov_out)."""
        d = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1)
        mu_out = mu_hist if mu_out is None else mu_out
        cov_out = cov_hist if cov_out is None else (None if cov_out is False else cov_out)
        _chk(self._lib.ukfb_smooth_dev(self._h, C.c_int(d.size + 1), _pd(d), C.c_int(slots), C.c_int(first_slot), _devptr(mu_hist),
                                       _devptr(cov_hist), _devptr(in_a_dev), _devptr(in_b_dev), _devptr(mu_out), _devptr(cov_out),
                                       _devptr(status)), "ukfb_smooth_dev")
        return mu_out, cov_out

    def smooth(self, dt, mu, cov, in_a=None, in_b=None):
        """Host arrays in window order: mu [steps, capacity, S], cov [steps, capacity, D, D], dt [steps - 1], in_a / in_b
        [steps, capacity, 3] or None -> (mu_s, cov_s, status [capacity]); synchronises"""
        d = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1)
        steps, n = d.size + 1, self.capacity
        mu = _f64(mu, (steps, n, self.S)).copy(); cov = _f64(cov, (steps, n, self.D, self.D)).copy()
        a = _f64(in_a, (steps, n, 3)) if in_a is not None else None
        b = _f64(in_b, (steps, n, 3)) if in_b is not None else None
        st = np.zeros(n, dtype=np.uint32)
        _chk(self._lib.ukfb_smooth(self._h, C.c_int(steps), _pd(d), _pd(mu), _pd(cov), _pd(a), _pd(b), _pu32(st)), "ukfb_smooth")
        return mu, cov, st

    # ---- forecast: rings [slots, capacity, S] / [slots, capacity, PK] in engine precision, the history's format
    @staticmethod
    def _forecast_steps(dt, ts_us):
        if (dt is None) == (ts_us is None):
            raise UkfbError("forecast: exactly one of dt and ts_us")
        d = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1) if dt is not None else None
        t = np.ascontiguousarray(ts_us, dtype=np.int64).reshape(-1) if ts_us is not None else None
        return d, t, (d.size if d is not None else t.size), _pi64(t)

    def forecast_dev(self, slots: int, first_slot: int, mu_out, cov_out=None, status=None, dt=None, ts_us=None, start_mu=None,
                     start_cov=None, in_a_dev=None, in_b_dev=None):
        """len(dt) (or len(ts_us)) predictions chained from the start record (start_mu / start_cov [capacity, S] /
        [capacity, PK] on the device, None = the engine's current state) WITHOUT committing them: step c, the state after
        c + 1 predictions, goes to slot (first_slot + c) % slots of mu_out / cov_out (cov_out may be None).  dt[c] (host) is
        the time step of every filter; ts_us[c] (host) a stamp that every filter measures against its OWN last measurement
        time, as predict_timestamps would on a copy.  in_a_dev / in_b_dev: input rings [slots, capacity, 3] (the slot of step c
        = the inputs of the prediction that produces it) or None (the latched inputs, held over the horizon); status uint32 /
        int32 [capacity] or None.  At most 32 steps a call; chain a longer horizon through start_mu / start_cov.
        Caller-supplied buffers: nothing is allocated.  Read-only on the engine.  Returns (mu_out, cov_out)."""
        d, t, steps, tp = self._forecast_steps(dt, ts_us)
        _chk(self._lib.ukfb_forecast_dev(self._h, C.c_int(steps), _pd(d), tp, C.c_int(slots), C.c_int(first_slot),
                                         _devptr(start_mu), _devptr(start_cov), _devptr(in_a_dev), _devptr(in_b_dev),
                                         _devptr(mu_out), _devptr(cov_out), _devptr(status)), "ukfb_forecast_dev")
        return mu_out, cov_out

    def forecast(self, dt=None, ts_us=None, start_mu=None, start_cov=None, in_a=None, in_b=None, with_cov: bool = True):
        """Host arrays in window order: dt or ts_us [steps], start_mu [capacity, S] and start_cov [capacity, D, D] (None: the
        engine's state), in_a / in_b [steps, capacity, 3] or None -> (mu [steps, capacity, S], cov [steps, capacity, D, D] or
        None, status [capacity]); synchronises"""
        d, t, steps, tp = self._forecast_steps(dt, ts_us)
        n = self.capacity
        sm = _f64(start_mu, (n, self.S)) if start_mu is not None else None
        sc = _f64(start_cov, (n, self.D, self.D)) if start_cov is not None else None
        a = _f64(in_a, (steps, n, 3)) if in_a is not None else None
        b = _f64(in_b, (steps, n, 3)) if in_b is not None else None
        mu = np.zeros((steps, n, self.S))
        cov = np.zeros((steps, n, self.D, self.D)) if with_cov else None
        st = np.zeros(n, dtype=np.uint32)
        _chk(self._lib.ukfb_forecast(self._h, C.c_int(steps), _pd(d), tp, _pd(sm), _pd(sc), _pd(a), _pd(b), _pd(mu), _pd(cov),
                                     _pu32(st)), "ukfb_forecast")
        return mu, cov, st

    # ---- filter lifecycle: records [n, S] / [n, PK] / int64 [n] / uint8 [n] / [n, 3] / [n, 3] / [n, D, D] / uint32 [n] on the device
    @staticmethod
    def _records(mu, cov_packed, last_ts_us, initialised, in_a, in_b, noise, status):
        rec = FilterRecords()
        for name, x in (("mu", mu), ("cov_packed", cov_packed), ("last_ts_us", last_ts_us), ("initialised", initialised),
                        ("in_a", in_a), ("in_b", in_b), ("noise", noise), ("status", status)):
            p = _devptr(x)
            setattr(rec, name, p.value if p is not None else None)
        return rec

    @staticmethod
    def _items(index_dev, n, capacity):
        if n is None:
            n = int(index_dev.numel()) if hasattr(index_dev, "numel") else (capacity if index_dev is None else None)
        if n is None:
            raise UkfbError("n is needed with an index given as a device address")
        return n

    def gather_filters_dev(self, index_dev, mu=None, cov_packed=None, last_ts_us=None, initialised=None, in_a=None, in_b=None,
                           noise=None, status=None, n: Optional[int] = None):
        """Record k <- filter index_dev[k] (int32 on the device; None: item k is filter k), field by field, None = skipped:
        mu [n, S], cov_packed [n, PK], last_ts_us int64 [n], initialised uint8 [n], in_a / in_b [n, 3] (what the filter's next
        prediction would read), noise [n, D, D], status uint32 / int32 [n].  An index outside [0, capacity) writes zeros and
        ST_INACTIVE.  Read-only on the engine; stream-ordered, no synchronisation.  Tensors or device addresses (then n)."""
        n = self._items(index_dev, n, self.capacity)
        rec = self._records(mu, cov_packed, last_ts_us, initialised, in_a, in_b, noise, status)
        _chk(self._lib.ukfb_gather_filters_dev(self._h, C.c_int64(n), _devptr(index_dev), C.byref(rec)), "ukfb_gather_filters_dev")

    def scatter_filters_dev(self, index_dev, mu, cov_packed, last_ts_us=None, initialised=None, in_a=None, in_b=None, noise=None,
                            status=None, n: Optional[int] = None):
        """initializeFilter from device records: filter index_dev[k] <- record k.  mu and cov_packed are required;
        initialised None = 1 (a 0 retires the filter), last_ts_us None = 0; in_a / in_b go into the engine's latches, noise into
        the filter's per-filter entry (the engine must already store its noise per filter).  Among the items that name one
        filter the lowest wins; every other one, and every index outside [0, capacity), gets ST_INACTIVE in status.
        Stream-ordered, no synchronisation."""
        n = self._items(index_dev, n, self.capacity)
        rec = self._records(mu, cov_packed, last_ts_us, initialised, in_a, in_b, noise, status)
        _chk(self._lib.ukfb_scatter_filters_dev(self._h, C.c_int64(n), _devptr(index_dev), C.byref(rec)), "ukfb_scatter_filters_dev")

    def retire_dev(self, retire_mask_dev):
        """uint8 / bool [capacity] on the device: a non-zero byte clears the filter's initialised flag and last measurement time"""
        _chk(self._lib.ukfb_retire_dev(self._h, _devptr(retire_mask_dev)), "ukfb_retire_dev")

    def compact_dev(self, group: int = 1, new_index=None, old_index=None, live=None):
        """Move the live groups of `group` consecutive filters to the front, in place (include/ukf_batch.h, "filter
        lifecycle").  new_index / old_index int32 [capacity] and live int64 [1] on the device, each may be None.  Bound input
        buffers are not moved: permute them with old_index."""
        _chk(self._lib.ukfb_compact_dev(self._h, C.c_int(group), _devptr(new_index), _devptr(old_index), _devptr(live)),
             "ukfb_compact_dev")

    def gather_filters(self, index=None, n: Optional[int] = None):
        """Host form: index int32 [n] or None (item k is filter k) -> (mu [n, S], cov [n, D, D], last_ts_us [n],
        initialised bool [n]); synchronises"""
        idx = np.ascontiguousarray(index, dtype=np.int32).reshape(-1) if index is not None else None
        n = (idx.size if idx is not None else self.capacity) if n is None else n
        mu, cov = np.zeros((n, self.S)), np.zeros((n, self.D, self.D))
        ts, init = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint8)
        _chk(self._lib.ukfb_gather_filters(self._h, C.c_int64(n), _pi32(idx), _pd(mu), _pd(cov), _pi64(ts), _pu8(init)),
             "ukfb_gather_filters")
        return mu, cov, ts, init.astype(bool)

    def scatter_filters(self, index, mu, cov, last_ts_us=None, initialised=None):
        """Host form: filter index[k] <- (mu[k], cov[k] full D x D, last_ts_us[k] or 0, initialised[k] or 1); returns the
        per-item status; synchronises"""
        mu = _f64(mu, (-1, self.S)); cov = _f64(cov, (-1, self.D, self.D))
        n = mu.shape[0]
        idx = np.ascontiguousarray(index, dtype=np.int32).reshape(-1) if index is not None else None
        ts = np.ascontiguousarray(last_ts_us, dtype=np.int64).reshape(n) if last_ts_us is not None else None
        init = np.ascontiguousarray(initialised, dtype=np.uint8).reshape(n) if initialised is not None else None
        if idx is not None and idx.size != n:
            raise UkfbError("scatter_filters: one index per record")
        st = np.zeros(n, dtype=np.uint32)
        _chk(self._lib.ukfb_scatter_filters(self._h, C.c_int64(n), _pi32(idx), _pd(mu), _pd(cov), _pi64(ts), _pu8(init), _pu32(st)),
             "ukfb_scatter_filters")
        return st

    def compact(self, group: int = 1):
        """Host form -> (new_index int32 [capacity], old_index int32 [capacity], live); synchronises"""
        new, old = np.zeros(self.capacity, dtype=np.int32), np.zeros(self.capacity, dtype=np.int32)
        live = C.c_int64(0)
        _chk(self._lib.ukfb_compact(self._h, C.c_int(group), _pi32(new), _pi32(old), C.byref(live)), "ukfb_compact")
        return new, old, int(live.value)

    # ---- joint state-block measurements: z in the state's own layout [capacity, S], Qz the packed lower triangle [capacity, PK]
    def update_state_dev(self, block_mask: int, z_dev, Qz_packed_dev, block_mask_dev=None, state_inflation: float = 1.0,
                         meas_inflation: float = 1.0, commit: bool = True, maha=None, loglik=None, status=None):
        """ukfom's update with the blocks `block_mask` selects as ONE measurement with its full covariance (BLOCK_* constants;
        block_mask_dev int32 [capacity] = a mask per filter, <= 0: none).  A record of device_views, a history slot or
        bank_combine_dev is a valid (z_dev, Qz_packed_dev) as it lies.  The update runs on state_inflation * Sigma and
        meas_inflation * Qz (1 / w, 1 / (1 - w): covariance intersection).  commit=False is read-only: only the keyword
        outputs (device buffers [capacity] in engine precision, status uint32 / int32) are written.  Stream-ordered."""
        out = StateMeasOut(_ptr(maha), _ptr(loglik), _ptr(status))
        _chk(self._lib.ukfb_update_state_dev(self._h, C.c_uint32(int(block_mask)), _devptr(block_mask_dev), _devptr(z_dev),
                                             _devptr(Qz_packed_dev), C.c_double(state_inflation), C.c_double(meas_inflation),
                                             C.c_int(1 if commit else 0), C.byref(out)), "ukfb_update_state_dev")

    def update_state(self, block_mask, z, Qz, state_inflation: float = 1.0, meas_inflation: float = 1.0, commit: bool = True):
        """Host arrays: z [capacity, S], Qz [capacity, D, D]; block_mask an int or an int32 array [capacity].  Returns
        (maha [capacity], loglik [capacity], status [capacity]); synchronises"""
        n = self.capacity
        z = _f64(z, (n, self.S)); Qz = _f64(Qz, (n, self.D, self.D))
        mask, per = _int_or_i32(block_mask, n)
        maha, ll, st = np.empty(n), np.empty(n), np.empty(n, dtype=np.uint32)
        _chk(self._lib.ukfb_update_state(self._h, C.c_uint32(mask), _pi32(per), _pd(z), _pd(Qz), C.c_double(state_inflation),
                                         C.c_double(meas_inflation), C.c_int(1 if commit else 0), _pd(maha), _pd(ll), _pu32(st)),
             "ukfb_update_state")
        return maha, ll, st

    def update_body_states(self, block_mask: int, records, active=None):
        """Pose engines: [capacity, 49] RigidBodyState records (the shape of export_body_states) integrated as measurements
        of the blocks `block_mask` selects; active uint8 [capacity] or None.  Synchronises."""
        rec = _f64(records, (self.capacity, BODY_STATE_SCALARS))
        act = np.ascontiguousarray(active, dtype=np.uint8).reshape(self.capacity) if active is not None else None
        _chk(self._lib.ukfb_pose_update_body_states(self._h, C.c_uint32(int(block_mask)), _pd(rec), _pu8(act)),
             "ukfb_pose_update_body_states")

    # ---- sensor-frame measurements: z [capacity, 3], Q [capacity, 9] (or 9 scalars), mount [capacity, 7], point [capacity, 3]
    def update_sensor_dev(self, model: int, z_dev, Q_dev, q_is_uniform: bool = False, model_dev=None, mount_dev=None,
                          mount=SENSOR_MOUNT_IDENTITY, point_dev=None, point=(0.0, 0.0, 0.0), commit: bool = True, z_pred=None,
                          S=None, innov=None, maha=None, loglik=None, status=None):
        """ukfom's update through a sensor-frame model (SENSOR_* constants; model_dev int32 [capacity] = an id per filter,
        negative: none).  mount = r[3] then qs[4] (x, y, z, w), point = b[3]: host values for the whole batch, or device
        arrays per filter (mount_dev / point_dev).  commit=False is read-only: only the keyword outputs (device buffers in
        engine precision, status uint32 / int32) are written.  Stream-ordered."""
        sin = SensorIn(_ptr(model_dev), _ptr(z_dev), _ptr(Q_dev), 1 if q_is_uniform else 0, _ptr(mount_dev),
                       (C.c_double * 7)(*[float(v) for v in mount]), _ptr(point_dev), (C.c_double * 3)(*[float(v) for v in point]))
        out = SensorOut(_ptr(z_pred), _ptr(S), _ptr(innov), _ptr(maha), _ptr(loglik), _ptr(status))
        _chk(self._lib.ukfb_update_sensor_dev(self._h, C.c_int(int(model)), C.byref(sin), C.c_int(1 if commit else 0), C.byref(out)),
             "ukfb_update_sensor_dev")

    def _update_sensor_frame(self, fn: str, model, z, Q, mount, point, commit):
        """ukfb_update_sensor and ukfb_update_bearing: one signature, one shape of arguments and results"""
        n = self.capacity
        z = _f64(z, (n, 3)); Q = _f64(Q, (n, 3, 3))
        uniform, per = _int_or_i32(model, n)
        mp, mu_ = _per_or_uniform(mount, n, 7)
        pp, pu = _per_or_uniform(point, n, 3)
        o = {"z_pred": np.empty((n, 3)), "S": np.empty((n, 3, 3)), "innov": np.empty((n, 3)), "maha": np.empty(n),
             "loglik": np.empty(n), "status": np.empty(n, dtype=np.uint32)}
        _chk(getattr(self._lib, fn)(self._h, C.c_int(uniform), _pi32(per), _pd(z), _pd(Q), _pd(mp), _pd(mu_), _pd(pp), _pd(pu),
                                    C.c_int(1 if commit else 0), _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]), _pd(o["maha"]),
                                    _pd(o["loglik"]), _pu32(o["status"])), fn)
        return o

    def update_sensor(self, model, z, Q, mount=SENSOR_MOUNT_IDENTITY, point=(0.0, 0.0, 0.0), commit: bool = True):
        """Host arrays: z [capacity, 3], Q [capacity, 3, 3]; model an int or an int32 array [capacity]; mount [7] or
        [capacity, 7], point [3] or [capacity, 3].  Returns a dict of NumPy arrays: z_pred [n, 3], S [n, 3, 3], innov [n, 3],
        maha [n], loglik [n], status [n]; synchronises"""
        return self._update_sensor_frame("ukfb_update_sensor", model, z, Q, mount, point, commit)

    # ---- bearing measurements: z [capacity, 3] a direction, Q [capacity, 9] (or 9 scalars), mount [capacity, 7], point [capacity, 3]
    def update_bearing_dev(self, model: int, z_dev, Q_dev, q_is_uniform: bool = False, model_dev=None, mount_dev=None,
                           mount=SENSOR_MOUNT_IDENTITY, point_dev=None, point=(0.0, 0.0, 0.0), commit: bool = True, z_pred=None,
                           S=None, innov=None, maha=None, loglik=None, status=None):
        """ukfom's update with a direction on the sphere S^2 (BEARING_* constants; model_dev int32 [capacity] = an id per
        filter, negative: none).  z need not be normalised; Q is the 3 x 3 covariance of the direction noise in the sensor
        frame, of which the tangent part at the predicted direction enters.  mount, point, commit and the keyword outputs as
        for update_sensor_dev; z_pred is a unit vector, S = Sigma_z + P Q P (3 x 3, rank 2), innov the sphere logarithm.
        Stream-ordered."""
        sin = SensorIn(_ptr(model_dev), _ptr(z_dev), _ptr(Q_dev), 1 if q_is_uniform else 0, _ptr(mount_dev),
                       (C.c_double * 7)(*[float(v) for v in mount]), _ptr(point_dev), (C.c_double * 3)(*[float(v) for v in point]))
        out = SensorOut(_ptr(z_pred), _ptr(S), _ptr(innov), _ptr(maha), _ptr(loglik), _ptr(status))
        _chk(self._lib.ukfb_update_bearing_dev(self._h, C.c_int(int(model)), C.byref(sin), C.c_int(1 if commit else 0), C.byref(out)),
             "ukfb_update_bearing_dev")

    def update_bearing(self, model, z, Q, mount=SENSOR_MOUNT_IDENTITY, point=(0.0, 0.0, 0.0), commit: bool = True):
        """Host arrays, shaped as for update_sensor.  Returns a dict of NumPy arrays: z_pred [n, 3], S [n, 3, 3], innov [n, 3],
        maha [n], loglik [n], status [n]; synchronises"""
        return self._update_sensor_frame("ukfb_update_bearing", model, z, Q, mount, point, commit)

    # ---- sensor-frame association: z [candidates, capacity, 3]; the point [capacity, 3] or, per hypothesis, [candidates, capacity, 3]
    def associate_sensor_dev(self, model: int, candidates: int, z_dev, Q_dev, q_is_uniform: bool = False, model_dev=None,
                             mount_dev=None, mount=SENSOR_MOUNT_IDENTITY, point_dev=None, point=(0.0, 0.0, 0.0),
                             point_per_candidate: bool = False, commit: bool = True, z_pred=None, S=None, innov=None, maha=None,
                             loglik=None, best=None, n_gated=None, status=None):
        """`candidates` samples per filter scored through a sensor-frame model (SENSOR_* constants) in one launch; the
        candidate with the smallest d^2 inside the gate is `best` and, with commit=True, updates the filter.
        point_per_candidate=False: every candidate is a detection of the one point (point_dev [capacity, 3] or the host
        value `point`); True: candidate k is a fix of its own landmark or beacon point_dev [candidates, capacity, 3].
        Keyword outputs (device buffers in engine precision; best, n_gated int32; status uint32 / int32): z_pred
        [H, capacity, 3], S [H, capacity, 9] with H = candidates per hypothesis, else 1; innov [candidates, capacity, 3],
        maha / loglik [candidates, capacity].  commit=False is read-only.  Stream-ordered."""
        ain = AssociateIn(_ptr(model_dev), int(candidates), _ptr(z_dev), _ptr(Q_dev), 1 if q_is_uniform else 0, _ptr(mount_dev),
                          (C.c_double * 7)(*[float(v) for v in mount]), _ptr(point_dev), (C.c_double * 3)(*[float(v) for v in point]),
                          1 if point_per_candidate else 0)
        out = AssociateOut(_ptr(z_pred), _ptr(S), _ptr(innov), _ptr(maha), _ptr(loglik), _ptr(best), _ptr(n_gated), _ptr(status))
        _chk(self._lib.ukfb_associate_sensor_dev(self._h, C.c_int(int(model)), C.byref(ain), C.c_int(1 if commit else 0), C.byref(out)),
             "ukfb_associate_sensor_dev")

    def associate_sensor(self, model, z, Q, mount=SENSOR_MOUNT_IDENTITY, point=(0.0, 0.0, 0.0), point_per_candidate: bool = False,
                         commit: bool = True):
        """Host arrays: z [candidates, capacity, 3], Q [capacity, 3, 3]; model an int or an int32 array [capacity]; mount [7]
        or [capacity, 7]; point [3] or [capacity, 3], with point_per_candidate [candidates, capacity, 3].  Returns a dict of
        NumPy arrays: z_pred [H, n, 3], S [H, n, 3, 3], innov [K, n, 3], maha / loglik [K, n], best / n_gated / status [n];
        synchronises"""
        n = self.capacity
        z = _f64(z)
        K = int(z.shape[0]) if z.ndim == 3 else 0
        z = _f64(z, (K, n, 3)); Q = _f64(Q, (n, 3, 3))
        H = K if point_per_candidate else 1
        uniform, per = _int_or_i32(model, n)
        mp, mu_ = _per_or_uniform(mount, n, 7)
        pp, pu = (_f64(point, (K, n, 3)), None) if point_per_candidate else _per_or_uniform(point, n, 3)
        o = {"z_pred": np.empty((H, n, 3)), "S": np.empty((H, n, 3, 3)), "innov": np.empty((K, n, 3)), "maha": np.empty((K, n)),
             "loglik": np.empty((K, n)), "best": np.empty(n, dtype=np.int32), "n_gated": np.empty(n, dtype=np.int32),
             "status": np.empty(n, dtype=np.uint32)}
        _chk(self._lib.ukfb_associate_sensor(self._h, C.c_int(uniform), _pi32(per), C.c_int(K), _pd(z), _pd(Q), _pd(mp), _pd(mu_),
                                             _pd(pp), _pd(pu), C.c_int(1 if point_per_candidate else 0),
                                             C.c_int(1 if commit else 0), _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]),
                                             _pd(o["maha"]), _pd(o["loglik"]), _pi32(o["best"]), _pi32(o["n_gated"]),
                                             _pu32(o["status"])), "ukfb_associate_sensor")
        return o

    # ---- user-defined measurement models: X [capacity, 2 D + 1, S], delta [capacity, 2 D + 1, D], Z [capacity, 2 D + 1, m]
    def sigma_points_dev(self, X_out=None, delta_out=None, status=None):
        """The sigma points of every filter into device buffers in engine precision, filter-major: X_out [capacity, 2 D + 1, S]
        (point 0 = mu, 1 + 2 j = mu (+) L col j, 2 + 2 j = mu (+) (-L col j)), delta_out [capacity, 2 D + 1, D] the tangent
        offsets themselves; either may be None, not both.  status uint32 / int32 [capacity] or None: 0, ST_UNINITIALISED or
        ST_ERR_CHOLESKY (rows of NaN).  Read-only on the engine.  Stream-ordered."""
        _chk(self._lib.ukfb_sigma_points_dev(self._h, _devptr(X_out), _devptr(delta_out), _devptr(status)), "ukfb_sigma_points_dev")

    def update_sampled_dev(self, m: int, Z_dev, z_dev, Q_dev, q_is_uniform: bool = False, active_dev=None, commit: bool = True,
                           z_pred=None, S=None, innov=None, maha=None, loglik=None, status=None):
        """ukfom's update finished from the caller's samples Z_dev [capacity, 2 D + 1, m] = h(X) of sigma_points_dev's X
        (m = 1 ... SAMPLED_MAX_M); z_dev [capacity, m], Q_dev [capacity, m, m] (one m x m with q_is_uniform), active_dev uint8
        [capacity] or None.  The state must not change between the export and this call.  z and Z may be written relative to
        any per-filter origin (fp32 engines: one near the values).  commit=False is read-only: only the keyword outputs
        (device buffers in engine precision, status uint32 / int32) are written.  Stream-ordered."""
        sin = SampledIn(int(m), _ptr(Z_dev), _ptr(z_dev), _ptr(Q_dev), 1 if q_is_uniform else 0, _ptr(active_dev))
        out = SampledOut(_ptr(z_pred), _ptr(S), _ptr(innov), _ptr(maha), _ptr(loglik), _ptr(status))
        _chk(self._lib.ukfb_update_sampled_dev(self._h, C.byref(sin), C.c_int(1 if commit else 0), C.byref(out)),
             "ukfb_update_sampled_dev")

    def sigma_points(self):
        """Host form -> (X [capacity, 2 D + 1, S], delta [capacity, 2 D + 1, D], status [capacity]); synchronises"""
        n, pts = self.capacity, 2 * self.D + 1
        X, delta, st = np.empty((n, pts, self.S)), np.empty((n, pts, self.D)), np.empty(n, dtype=np.uint32)
        _chk(self._lib.ukfb_sigma_points(self._h, _pd(X), _pd(delta), _pu32(st)), "ukfb_sigma_points")
        return X, delta, st

    def update_sampled(self, Z, z, Q, active=None, commit: bool = True):
        """Host arrays: Z [capacity, 2 D + 1, m], z [capacity, m], Q [capacity, m, m] or [m, m] (one for the batch); active
        uint8 [capacity] or None.  Returns a dict of NumPy arrays: z_pred [n, m], S [n, m, m], innov [n, m], maha [n],
        loglik [n], status [n]; synchronises"""
        n, pts = self.capacity, 2 * self.D + 1
        Z = _f64(Z)
        m = int(Z.shape[-1]) if Z.ndim == 3 else Z.size // max(n * pts, 1)
        Z = Z.reshape(n, pts, m); z = _f64(z, (n, m)); Q = _f64(Q)
        uniform = Q.ndim == 2
        Q = Q.reshape(m, m) if uniform else Q.reshape(n, m, m)
        act = np.ascontiguousarray(active, dtype=np.uint8).reshape(n) if active is not None else None
        o = {"z_pred": np.empty((n, m)), "S": np.empty((n, m, m)), "innov": np.empty((n, m)), "maha": np.empty(n),
             "loglik": np.empty(n), "status": np.empty(n, dtype=np.uint32)}
        _chk(self._lib.ukfb_update_sampled(self._h, C.c_int(m), _pd(Z), _pd(z), _pd(Q), C.c_int(1 if uniform else 0), _pu8(act),
                                           C.c_int(1 if commit else 0), _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]),
                                           _pd(o["maha"]), _pd(o["loglik"]), _pu32(o["status"])), "ukfb_update_sampled")
        return o

    # ---- user-defined process models: XX [capacity, 2 D + 1, S] = f(X) of sigma_points_dev's X, R [capacity, D, D]
    def predict_sampled_dev(self, XX, R, r_is_uniform: bool = False, active_dev=None, commit: bool = True, mu=None,
                            cov_packed=None, status=None):
        """ukfom's predict finished from the caller's propagated sigma points XX [capacity, 2 D + 1, S] = f(X) of
        sigma_points_dev's X and the caller's R [capacity, D, D] (one D x D with r_is_uniform; taken as given, the lower triangle
        is read); active_dev uint8 [capacity] or None.  Times, noise tables and latches are not touched.  commit=False is
        read-only: only the keyword outputs (device buffers in engine precision: mu [capacity, S], cov_packed [capacity, PK];
        status uint32 / int32) are written.  Stream-ordered, nothing is allocated."""
        pin = PredictSampledIn(_ptr(XX), _ptr(R), 1 if r_is_uniform else 0, _ptr(active_dev))
        out = PredictSampledOut(_ptr(mu), _ptr(cov_packed), _ptr(status))
        _chk(self._lib.ukfb_predict_sampled_dev(self._h, C.byref(pin), C.c_int(1 if commit else 0), C.byref(out)),
             "ukfb_predict_sampled_dev")

    def predict_sampled(self, XX, R, active=None, commit: bool = True):
        """Host arrays: XX [capacity, 2 D + 1, S], R [capacity, D, D] or [D, D] (one for the batch); active uint8 [capacity] or
        None.  Returns a dict of NumPy arrays: mu [n, S], cov [n, D, D], status [n]; synchronises"""
        n, pts, S, D = self.capacity, 2 * self.D + 1, self.S, self.D
        XX = _f64(XX, (n, pts, S)); R = _f64(R)
        uniform = R.ndim == 2
        R = R.reshape(D, D) if uniform else R.reshape(n, D, D)
        act = np.ascontiguousarray(active, dtype=np.uint8).reshape(n) if active is not None else None
        o = {"mu": np.empty((n, S)), "cov": np.empty((n, D, D)), "status": np.empty(n, dtype=np.uint32)}
        _chk(self._lib.ukfb_predict_sampled(self._h, _pd(XX), _pd(R), C.c_int(1 if uniform else 0), _pu8(act),
                                            C.c_int(1 if commit else 0), _pd(o["mu"]), _pd(o["cov"]), _pu32(o["status"])),
             "ukfb_predict_sampled")
        return o

    # ---- covariance conditioning: var_floor [D], eig_floor in (0, 1)
    def condition_dev(self, var_floor_dev, eig_floor: float, select_dev=None, renormalize_quaternion: bool = False, commit: bool = True,
                      eig_min=None, eig_max=None, mu=None, cov_packed=None, status=None):
        """Eigenvalue repair of every selected filter's covariance in its correlation scaling (include/ukf_batch.h, "covariance
        conditioning"): var_floor_dev [D] a device buffer in engine precision, eig_floor the floor of the correlation eigenvalues
        (1e-4 suits fp32 storage, 1e-10 fp64), select_dev uint8 [capacity] or None.  A filter whose smallest correlation
        eigenvalue is below eig_floor / 2, or one of whose variances is below the floor, is repaired (ST_REPAIRED); a healthy one
        keeps every bit.  renormalize_quaternion also brings the stored quaternion back to unit length.  commit=False is
        read-only: only the keyword outputs (device buffers in engine precision: eig_min / eig_max [capacity], mu [capacity, S],
        cov_packed [capacity, PK]; status uint32 / int32) are written.  Stream-ordered, nothing is allocated."""
        cin = ConditionIn(_ptr(var_floor_dev), float(eig_floor), _ptr(select_dev), 1 if renormalize_quaternion else 0)
        out = ConditionOut(_ptr(eig_min), _ptr(eig_max), _ptr(mu), _ptr(cov_packed), _ptr(status))
        _chk(self._lib.ukfb_condition_dev(self._h, C.byref(cin), C.c_int(1 if commit else 0), C.byref(out)), "ukfb_condition_dev")

    def condition(self, var_floor, eig_floor: float, select=None, renormalize_quaternion: bool = False, commit: bool = True):
        """Host arrays: var_floor [D] (every entry finite and > 0), select uint8 [capacity] or None.  Returns a dict of NumPy
        arrays: eig_min [n], eig_max [n], mu [n, S], cov [n, D, D], status [n]; synchronises"""
        n, S, D = self.capacity, self.S, self.D
        v = _f64(var_floor, (D,))
        sel = np.ascontiguousarray(select, dtype=np.uint8).reshape(n) if select is not None else None
        o = {"eig_min": np.empty(n), "eig_max": np.empty(n), "mu": np.empty((n, S)), "cov": np.empty((n, D, D)),
             "status": np.empty(n, dtype=np.uint32)}
        _chk(self._lib.ukfb_condition(self._h, _pd(v), C.c_double(float(eig_floor)), _pu8(sel),
                                      C.c_int(1 if renormalize_quaternion else 0), C.c_int(1 if commit else 0), _pd(o["eig_min"]),
                                      _pd(o["eig_max"]), _pd(o["mu"]), _pd(o["cov"]), _pu32(o["status"])), "ukfb_condition")
        return o

    # ---- late samples: the window of smooth_dev with the engine's own state as its last step
    def update_delayed_dev(self, dt, slots: int, first_slot: int, mu_hist, cov_hist, lag, meas_model, z_dev, Q_dev,
                           q_is_uniform: bool = False, in_a_dev=None, in_b_dev=None, commit: bool = True, z_pred=None, S=None,
                           innov=None, maha=None, loglik=None, status=None, mu_out=None, cov_out=None):
        """A sample taken `lag` steps ago corrects the current state through the history ring (include/ukf_batch.h, "late
        samples").  The window has len(dt) + 1 steps, step c in slot (first_slot + c) % slots, the last step being the engine's
        own state (its slot is not read).  lag / meas_model: an int for the whole batch or an int32 device array [capacity].
        z_dev [capacity, 3], Q_dev [capacity, 9] (9 scalars with q_is_uniform).  commit=False is read-only: only the keyword
        outputs (device buffers in engine precision, status uint32 / int32; mu_out [capacity, S] / cov_out [capacity, PK] = the
        corrected present state) are written.  Stream-ordered, nothing is allocated."""
        d = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1)
        per = lambda x: (0, _ptr(x)) if hasattr(x, "data_ptr") else (int(x), None)
        (lag_u, lag_p), (mod_u, mod_p) = per(lag), per(meas_model)
        din = DelayedIn(d.size + 1, _pd(d) if d.size else None, int(slots), int(first_slot), _ptr(mu_hist), _ptr(cov_hist),
                        _ptr(in_a_dev), _ptr(in_b_dev), lag_u, lag_p, mod_u, mod_p, _ptr(z_dev), _ptr(Q_dev), 1 if q_is_uniform else 0)
        out = DelayedOut(_ptr(z_pred), _ptr(S), _ptr(innov), _ptr(maha), _ptr(loglik), _ptr(status), _ptr(mu_out), _ptr(cov_out))
        _chk(self._lib.ukfb_update_delayed_dev(self._h, C.byref(din), C.c_int(1 if commit else 0), C.byref(out)),
             "ukfb_update_delayed_dev")

    def update_delayed(self, dt, mu_hist, cov_hist, lag, meas_model, z, Q, in_a=None, in_b=None, commit: bool = True):
        """Host arrays in window order: mu_hist [steps, capacity, S], cov_hist [steps, capacity, D, D] (the last step is not
        read), dt [steps - 1], in_a / in_b [steps, capacity, 3] or None; lag / meas_model an int or an int32 array [capacity];
        z [capacity, 3], Q [capacity, 3, 3].  Returns a dict of NumPy arrays: z_pred [n, 4], S [n, 3, 3], innov [n, 3], maha,
        loglik, status [n], mu_out [n, S], cov_out [n, D, D]; synchronises"""
        d = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1)
        steps, n = d.size + 1, self.capacity
        mu_hist = _f64(mu_hist, (steps, n, self.S)); cov_hist = _f64(cov_hist, (steps, n, self.D, self.D))
        a = _f64(in_a, (steps, n, 3)) if in_a is not None else None
        b = _f64(in_b, (steps, n, 3)) if in_b is not None else None
        z = _f64(z, (n, 3)); Q = _f64(Q, (n, 3, 3))
        (lag_u, lag_p), (mod_u, mod_p) = _int_or_i32(lag, n), _int_or_i32(meas_model, n)
        o = {"z_pred": np.empty((n, 4)), "S": np.empty((n, 3, 3)), "innov": np.empty((n, 3)), "maha": np.empty(n),
             "loglik": np.empty(n), "status": np.empty(n, dtype=np.uint32), "mu_out": np.empty((n, self.S)),
             "cov_out": np.empty((n, self.D, self.D))}
        _chk(self._lib.ukfb_update_delayed(self._h, C.c_int(steps), _pd(d) if d.size else None, _pd(mu_hist), _pd(cov_hist),
                                           _pd(a), _pd(b), C.c_int(lag_u), _pi32(lag_p), C.c_int(mod_u), _pi32(mod_p), _pd(z), _pd(Q),
                                           C.c_int(1 if commit else 0), _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]),
                                           _pd(o["maha"]), _pd(o["loglik"]), _pu32(o["status"]), _pd(o["mu_out"]),
                                           _pd(o["cov_out"])), "ukfb_update_delayed")
        return o

    def delayed_lag_dev(self, step_ts_us, sample_ts_us_dev, lag_out_dev):
        """step_ts_us: host int64 stamps of the window's steps (strictly increasing); sample_ts_us_dev int64 [capacity] ->
        lag_out_dev int32 [capacity]: the step nearest each sample (ties: the older), 0 for a sample newer than the present,
        len(step_ts_us) (out of the window) for one older than the first step by more than half a step.  Stream-ordered."""
        ts = np.ascontiguousarray(step_ts_us, dtype=np.int64).reshape(-1)
        _chk(self._lib.ukfb_delayed_lag_dev(self._h, C.c_int(ts.size), _pi64(ts), _devptr(sample_ts_us_dev), _devptr(lag_out_dev)),
             "ukfb_delayed_lag_dev")

    # ---- fused cycle
    def cycle(self, dt: float, meas_model: int, z, Q):
        z = _f64(z, (self.capacity, 3)); Q = _f64(Q, (self.capacity, 3, 3))
        _chk(self._lib.ukfb_cycle(self._h, C.c_double(dt), C.c_int(meas_model), _pd(z), _pd(Q)), "ukfb_cycle")

    def cycle_uniform_q(self, dt: float, meas_model: int, z, Q9):
        """fused cycle with ONE 3x3 measurement covariance for the whole batch (host arrays)"""
        z = _f64(z, (self.capacity, 3)); Q9 = _f64(Q9, (9,))
        _chk(self._lib.ukfb_cycle_uniform_q(self._h, C.c_double(dt), C.c_int(meas_model), _pd(z), _pd(Q9)), "ukfb_cycle_uniform_q")

    def cycle_uniform_q_dev(self, dt: float, meas_model: int, z_dev, Q9_dev):
        _chk(self._lib.ukfb_cycle_uniform_q_dev(self._h, C.c_double(dt), C.c_int(meas_model), _devptr(z_dev), _devptr(Q9_dev)),
             "ukfb_cycle_uniform_q_dev")

    def update_uniform_q(self, meas_model: int, z, Q9, active=None):
        z = _f64(z, (self.capacity, 3)); Q9 = _f64(Q9, (9,))
        a = None if active is None else np.ascontiguousarray(active, dtype=np.uint8).reshape(self.capacity)
        _chk(self._lib.ukfb_update_uniform_q(self._h, C.c_int(meas_model), _pd(z), _pd(Q9), _pu8(a)), "ukfb_update_uniform_q")

    def cycle_dev(self, dt: float, meas_model_uniform: int, z_dev, Q_dev, meas_model_dev=None):
        _chk(self._lib.ukfb_cycle_dev(self._h, C.c_double(dt), C.c_int(meas_model_uniform), _devptr(meas_model_dev),
                                      _devptr(z_dev), _devptr(Q_dev)), "ukfb_cycle_dev")

    def cycle_multi_dev(self, cycles: int, dt: float, meas_model: int, z_dev, Q_dev, slots: int, first_slot: int = 0,
                        in_a_dev=None, in_b_dev=None):
        """`cycles` fused cycles in one launch, the filters stay in LDS in between; cycle c reads slot (first_slot + c) % slots
        of the device rings z_dev [slots][capacity][3], Q_dev [slots][capacity][9] and, if given, in_a_dev / in_b_dev
        [slots][capacity][3] (Pose: acceleration; Orient: acceleration, rotation rate) in place of the latched inputs."""
        _chk(self._lib.ukfb_cycle_multi_dev(self._h, C.c_int(cycles), C.c_double(dt), C.c_int(meas_model), C.c_int(slots),
                                            C.c_int(first_slot), _devptr(in_a_dev), _devptr(in_b_dev), _devptr(z_dev),
                                            _devptr(Q_dev)), "ukfb_cycle_multi_dev")

    def cycle_multi_mixed_dev(self, cycles: int, dt: float, meas_model_dev, z_dev, Q_dev, slots: int, first_slot: int = 0,
                              in_a_dev=None, in_b_dev=None):
        """cycle_multi_dev with per-filter model ids per cycle: meas_model_dev int32 [slots][capacity], negative = none."""
        _chk(self._lib.ukfb_cycle_multi_mixed_dev(self._h, C.c_int(cycles), C.c_double(dt), C.c_int(slots), C.c_int(first_slot),
                                                  _devptr(in_a_dev), _devptr(in_b_dev), _devptr(meas_model_dev),
                                                  _devptr(z_dev), _devptr(Q_dev)), "ukfb_cycle_multi_mixed_dev")

    def cycle_schedule_dev(self, dt, meas_model, z_dev, Q_dev, slots: int, first_slot: int = 0, in_a_dev=None, in_b_dev=None):
        """Scheduled multi-cycle launch: cycle c predicts by dt[c] and updates with model meas_model[c] (negative: prediction
        only); inputs from the device rings as in cycle_multi_dev."""
        d = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1)
        m = np.ascontiguousarray(meas_model, dtype=np.int32).reshape(-1)
        if d.size != m.size:
            raise ValueError("dt and meas_model need one entry per cycle")
        _chk(self._lib.ukfb_cycle_schedule_dev(self._h, C.c_int(d.size), _pd(d), _pi32(m), C.c_int(slots), C.c_int(first_slot),
                                               _devptr(in_a_dev), _devptr(in_b_dev), _devptr(z_dev), _devptr(Q_dev)),
             "ukfb_cycle_schedule_dev")

    def cycle_multi(self, dt: float, meas_model: int, z, Q, in_a=None, in_b=None):
        """Host arrays, one input set per cycle: z [cycles, capacity, 3], Q [cycles, capacity, 3, 3], in_a / in_b
        [cycles, capacity, 3] or None (the latched inputs); all cycles in one launch."""
        z = np.ascontiguousarray(z, dtype=np.float64)
        cycles = z.shape[0]
        z = _f64(z, (cycles, self.capacity, 3)); Q = _f64(Q, (cycles, self.capacity, 3, 3))
        a = None if in_a is None else _f64(in_a, (cycles, self.capacity, 3))
        b = None if in_b is None else _f64(in_b, (cycles, self.capacity, 3))
        _chk(self._lib.ukfb_cycle_multi(self._h, C.c_int(cycles), C.c_double(dt), C.c_int(meas_model),
                                        _pd(a) if a is not None else None, _pd(b) if b is not None else None, _pd(z), _pd(Q)),
             "ukfb_cycle_multi")

    def cycle_timestamps(self, ts_us, meas_model, z, Q):
        """Fused predictionStepFromSampleTime(ts[i]) + integrateMeasurement(model[i]); ts < 0: no sample."""
        t = np.ascontiguousarray(ts_us, dtype=np.int64).reshape(self.capacity)
        m = np.ascontiguousarray(meas_model, dtype=np.int32).reshape(self.capacity)
        z = _f64(z, (self.capacity, 3)); Q = _f64(Q, (self.capacity, 3, 3))
        _chk(self._lib.ukfb_cycle_timestamps(self._h, _pi64(t), _pi32(m), _pd(z), _pd(Q)), "ukfb_cycle_timestamps")

    def process_events(self, filter_index, ts_us, meas_model, z, Q):
        """Time-ordered asynchronous measurement stream (any arrival order).  Returns (status_or, rounds)."""
        f = np.ascontiguousarray(filter_index, dtype=np.int64).reshape(-1)
        n = f.size
        t = np.ascontiguousarray(ts_us, dtype=np.int64).reshape(n)
        m = np.ascontiguousarray(meas_model, dtype=np.int32).reshape(n)
        z = _f64(z, (n, 3)); Q = _f64(Q, (n, 3, 3))
        st, rounds = C.c_uint32(0), C.c_int64(0)
        _chk(self._lib.ukfb_process_events(self._h, C.c_int64(n), _pi64(f), _pi64(t), _pi32(m), _pd(z), _pd(Q), C.byref(st),
                                           C.byref(rounds)), "ukfb_process_events")
        return int(st.value), int(rounds.value)

    def process_events_dev(self, n_events: int, filter_dev, ts_us_dev, meas_model_dev, z_dev, Q_dev):
        """The same stream already resident in HBM (int64, int64, int32, z / Q in the engine's precision)."""
        st, rounds = C.c_uint32(0), C.c_int64(0)
        _chk(self._lib.ukfb_process_events_dev(self._h, C.c_int64(int(n_events)), _devptr(filter_dev), _devptr(ts_us_dev),
                                               _devptr(meas_model_dev), _devptr(z_dev), _devptr(Q_dev), C.byref(st),
                                               C.byref(rounds)), "ukfb_process_events_dev")
        return int(st.value), int(rounds.value)

    # ---- measurement of the engine
    def last_launch_info(self):
        name = C.create_string_buffer(256)
        lds, fpw, grid = C.c_int(0), C.c_int(0), C.c_int64(0)
        _chk(self._lib.ukfb_last_launch_info(self._h, name, C.c_int(256), C.byref(lds), C.byref(fpw), C.byref(grid)),
             "ukfb_last_launch_info")
        return {"kernel": name.value.decode(), "lds_bytes": lds.value, "filters_per_workgroup": fpw.value,
                "grid": grid.value}

    def last_model_groups(self):
        """int32 list of the most recent launch that grouped its filters by update class (-1 = padding); see ukf_batch.h"""
        items = C.c_int64(0)
        cap = int(self.capacity) + 16
        out = np.empty(cap, dtype=np.int32)
        _chk(self._lib.ukfb_last_model_groups(self._h, _pi32(out), C.c_int64(cap), C.byref(items)), "ukfb_last_model_groups")
        return out[:int(items.value)].copy()

    def timer_begin(self):
        _chk(self._lib.ukfb_timer_begin(self._h), "ukfb_timer_begin")

    def timer_end(self) -> float:
        ms = C.c_float(0)
        _chk(self._lib.ukfb_timer_end(self._h, C.byref(ms)), "ukfb_timer_end")
        return float(ms.value)


class BatchPoseUKF(BatchUKF):
    """Batched sibling of pose_estimation::PoseUKF (pose_with_velocity/PoseUKF.hpp:20-96)."""

    def __init__(self, capacity: int, precision: int = F64, device: int = 0, **kw):
        super().__init__(MODEL_POSE, precision, capacity, device, **kw)
        # PoseUKF ctor defaults (PoseUKF.cpp:103-107)
        self.set_process_noise(np.diag([0.01] * 3 + [0.001] * 3 + [0.00001] * 3 + [0.00001] * 3))


class BatchOrientationUKF(BatchUKF):
    """Batched sibling of pose_estimation::OrientationUKF (orientation_estimator/OrientationUKF.hpp:20-62)."""

    EARTHW = (2.0 * np.pi) / 86164.0  # GravitationalModel.hpp:16

    def __init__(self, capacity: int, gyro_bias_tau: float, acc_bias_tau: float, latitude: float,
                 precision: int = F64, device: int = 0, **kw):
        super().__init__(MODEL_ORIENT, precision, capacity, device, **kw)
        # OrientationUKF.cpp:47
        self.earth_rotation = np.array([self.EARTHW * np.cos(latitude), 0.0, self.EARTHW * np.sin(latitude)])
        self.set_orient_params(gyro_bias_tau, acc_bias_tau, self.earth_rotation)

    def initialize(self, mu, cov, first: int = 0):
        """initializeFilter plus the ctor's input latches (OrientationUKF.cpp:49-50)."""
        mu = _f64(mu, (-1, self.S))
        super().initialize(mu, cov, first)
        n = mu.shape[0]
        acc = np.zeros((n, 3)); acc[:, 2] = mu[:, 13]
        self.set_orient_inputs(gyro=np.zeros((n, 3)), acc=acc, first=first)


class _ShardView(BatchUKF):
    """A shard's engine seen through the per-engine binding (the group owns the handle: close() is a no-op)."""

    def __init__(self, lib, handle, model, precision, capacity, device):   # noqa: D401 (no ukfb_create here)
        self._lib, self._h = lib, handle
        self.model, self.precision, self.capacity, self.device = model, precision, int(capacity), device
        self.S = 13 if model == MODEL_POSE else 14
        self.D = 12 if model == MODEL_POSE else 13
        self.PK = self.D * (self.D + 1) // 2
        self.dtype = np.float64 if precision == F64 else np.float32
        self.stream_kind = "private"

    def close(self):
        self._h = C.c_void_p()


class UKFGroup:
    """One process, several GPUs: `total` independent filters in contiguous shards, one engine per device
    (ukfb_group_* of include/ukf_batch.h).  Mirrors pose_estimation::ShardedBatchPoseUKF (include/pose_estimation/Batch.hpp)."""

    def __init__(self, model: int, precision: int, total: int, devices):
        self._lib = load_library()
        self._g = C.c_void_p()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        _chk(self._lib.ukfb_group_create(C.byref(self._g), C.c_int(model), C.c_int(precision), C.c_int64(total), devs,
                                         C.c_int(len(devices))), "ukfb_group_create")
        self.model, self.precision, self.total = model, precision, int(total)
        self.S = 13 if model == MODEL_POSE else 14
        self.D = 12 if model == MODEL_POSE else 13
        self.n = int(self._lib.ukfb_group_size(self._g))
        self.shards = []
        for r in range(self.n):
            h, dev, first, count = C.c_void_p(), C.c_int(0), C.c_int64(0), C.c_int64(0)
            _chk(self._lib.ukfb_group_shard(self._g, C.c_int(r), C.byref(h), C.byref(dev), C.byref(first), C.byref(count)),
                 "ukfb_group_shard")
            self.shards.append({"engine": _ShardView(self._lib, h, model, precision, count.value, dev.value),
                                "device": dev.value, "first": first.value, "count": count.value})
        if model == MODEL_POSE:   # PoseUKF ctor defaults (PoseUKF.cpp:103-107), as BatchPoseUKF
            self.set_process_noise(np.diag([0.01] * 3 + [0.001] * 3 + [0.00001] * 3 + [0.00001] * 3))

    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            self._lib.ukfb_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ptrs(self, xs):
        if xs is None:
            return None
        assert len(xs) == self.n, "one device pointer per shard"
        return (C.c_void_p * self.n)(*[(_devptr(x).value if x is not None else None) for x in xs])

    def configure(self, **kw):
        c = self.shards[0]["engine"].config()
        for k, v in kw.items():
            setattr(c, k, v)
        _chk(self._lib.ukfb_group_set_config(self._g, C.byref(c)), "ukfb_group_set_config")

    def initialize(self, mu, cov, first: int = 0):
        mu = _f64(mu, (-1, self.S)); cov = _f64(cov, (-1, self.D, self.D))
        _chk(self._lib.ukfb_group_initialize(self._g, C.c_int64(first), C.c_int64(mu.shape[0]), _pd(mu), _pd(cov)),
             "ukfb_group_initialize")
        if self.model == MODEL_ORIENT:   # the reference constructor's input latches (OrientationUKF.cpp:49-50), as BatchOrientationUKF
            n = mu.shape[0]
            acc = np.zeros((n, 3)); acc[:, 2] = mu[:, 13]
            self.set_orient_inputs(gyro=np.zeros((n, 3)), acc=acc, first=first)

    def state(self, first: int = 0, count: Optional[int] = None):
        count = self.total - first if count is None else count
        mu = np.empty((count, self.S)); cov = np.empty((count, self.D, self.D)); init = np.empty(count, dtype=np.uint8)
        _chk(self._lib.ukfb_group_get_state(self._g, C.c_int64(first), C.c_int64(count), _pd(mu), _pd(cov), _pu8(init)),
             "ukfb_group_get_state")
        return mu, cov, init.astype(bool)

    def status(self, first: int = 0, count: Optional[int] = None):
        count = self.total - first if count is None else count
        st = np.empty(count, dtype=np.uint32)
        _chk(self._lib.ukfb_group_get_status(self._g, C.c_int64(first), C.c_int64(count), _pu32(st)), "ukfb_group_get_status")
        return st

    def status_summary(self) -> int:
        v = C.c_uint32(0)
        _chk(self._lib.ukfb_group_get_status_summary(self._g, C.byref(v)), "ukfb_group_get_status_summary")
        return int(v.value)

    def set_process_noise(self, R):
        _chk(self._lib.ukfb_group_set_process_noise(self._g, _pd(_f64(R, (self.D, self.D)))), "ukfb_group_set_process_noise")

    def set_acceleration(self, acc_mu=None, acc_cov=None, first: int = 0):
        am = _f64(acc_mu, (-1, 3)) if acc_mu is not None else None
        ac = _f64(acc_cov, (3, 3)) if acc_cov is not None else None
        _chk(self._lib.ukfb_group_pose_set_acceleration(self._g, C.c_int64(first), C.c_int64(am.shape[0] if am is not None else 0),
                                                        _pd(am), _pd(ac)), "ukfb_group_pose_set_acceleration")

    def set_orient_params(self, gyro_bias_tau: float, acc_bias_tau: float, earth_rotation):
        _chk(self._lib.ukfb_group_orient_set_params(self._g, C.c_double(gyro_bias_tau), C.c_double(acc_bias_tau),
                                                    _pd(_f64(earth_rotation, (3,)))), "ukfb_group_orient_set_params")

    def set_orient_inputs(self, gyro=None, acc=None, first: int = 0):
        g = _f64(gyro, (-1, 3)) if gyro is not None else None
        a = _f64(acc, (-1, 3)) if acc is not None else None
        n = g.shape[0] if g is not None else (a.shape[0] if a is not None else 0)
        _chk(self._lib.ukfb_group_orient_set_inputs(self._g, C.c_int64(first), C.c_int64(n), _pd(g), _pd(a)),
             "ukfb_group_orient_set_inputs")

    def predict(self, dt: float):
        _chk(self._lib.ukfb_group_predict(self._g, C.c_double(dt)), "ukfb_group_predict")

    def update(self, meas_model: int, z, Q):
        z = _f64(z, (self.total, 3)); Q = _f64(Q, (self.total, 3, 3))
        _chk(self._lib.ukfb_group_update(self._g, C.c_int(meas_model), _pd(z), _pd(Q)), "ukfb_group_update")

    def cycle(self, dt: float, meas_model: int, z, Q):
        z = _f64(z, (self.total, 3)); Q = _f64(Q, (self.total, 3, 3))
        _chk(self._lib.ukfb_group_cycle(self._g, C.c_double(dt), C.c_int(meas_model), _pd(z), _pd(Q)), "ukfb_group_cycle")

    def bind_acceleration_dev(self, acc_devs):
        _chk(self._lib.ukfb_group_pose_bind_acceleration_dev(self._g, self._ptrs(acc_devs)), "ukfb_group_pose_bind_acceleration_dev")

    def bind_orient_inputs_dev(self, gyro_devs, acc_devs):
        _chk(self._lib.ukfb_group_orient_bind_inputs_dev(self._g, self._ptrs(gyro_devs), self._ptrs(acc_devs)),
             "ukfb_group_orient_bind_inputs_dev")

    def cycle_dev(self, dt: float, meas_model: int, z_devs, Q_devs):
        _chk(self._lib.ukfb_group_cycle_dev(self._g, C.c_double(dt), C.c_int(meas_model), self._ptrs(z_devs), self._ptrs(Q_devs)),
             "ukfb_group_cycle_dev")

    def cycle_multi_dev(self, cycles: int, dt: float, meas_model: int, z_devs, Q_devs, slots: int, first_slot: int = 0,
                        in_a_devs=None, in_b_devs=None):
        _chk(self._lib.ukfb_group_cycle_multi_dev(self._g, C.c_int(cycles), C.c_double(dt), C.c_int(meas_model), C.c_int(slots),
                                                  C.c_int(first_slot), self._ptrs(in_a_devs), self._ptrs(in_b_devs),
                                                  self._ptrs(z_devs), self._ptrs(Q_devs)), "ukfb_group_cycle_multi_dev")

    def cycle_mixed_dev(self, dt: float, meas_model_devs, z_devs, Q_devs):
        """per-filter model ids resident on the devices (int32, one array per shard)"""
        _chk(self._lib.ukfb_group_cycle_mixed_dev(self._g, C.c_double(dt), self._ptrs(meas_model_devs), self._ptrs(z_devs),
                                                  self._ptrs(Q_devs)), "ukfb_group_cycle_mixed_dev")

    def cycle_timestamps(self, ts_us, meas_model, z, Q):
        t = np.ascontiguousarray(ts_us, dtype=np.int64).reshape(self.total)
        m = np.ascontiguousarray(meas_model, dtype=np.int32).reshape(self.total)
        z = _f64(z, (self.total, 3)); Q = _f64(Q, (self.total, 3, 3))
        _chk(self._lib.ukfb_group_cycle_timestamps(self._g, _pi64(t), _pi32(m), _pd(z), _pd(Q)), "ukfb_group_cycle_timestamps")

    def process_events(self, filter_index, ts_us, meas_model, z, Q):
        """Time-ordered asynchronous stream over the sharded batch (filter indices in batch numbering, any arrival order).
        Returns (status_or, rounds of the shard that needed most)."""
        f = np.ascontiguousarray(filter_index, dtype=np.int64).reshape(-1)
        n = f.size
        t = np.ascontiguousarray(ts_us, dtype=np.int64).reshape(n)
        m = np.ascontiguousarray(meas_model, dtype=np.int32).reshape(n)
        z = _f64(z, (n, 3)); Q = _f64(Q, (n, 3, 3))
        st, rounds = C.c_uint32(0), C.c_int64(0)
        _chk(self._lib.ukfb_group_process_events(self._g, C.c_int64(n), _pi64(f), _pi64(t), _pi32(m), _pd(z), _pd(Q), C.byref(st),
                                                 C.byref(rounds)), "ukfb_group_process_events")
        return int(st.value), int(rounds.value)

    def sync(self):
        _chk(self._lib.ukfb_group_sync(self._g), "ukfb_group_sync")

    def timer_begin(self):
        _chk(self._lib.ukfb_group_timer_begin(self._g), "ukfb_group_timer_begin")

    def timer_end(self):
        """(slowest shard's ms, [ms per shard])"""
        mx = C.c_float(0)
        per = (C.c_float * self.n)()
        _chk(self._lib.ukfb_group_timer_end(self._g, C.byref(mx), per), "ukfb_group_timer_end")
        return float(mx.value), [float(x) for x in per]

    def gather_means(self, out_devs):
        """RCCL all-gather of the means: out_devs[r] = device buffer [total][S] (engine precision) on shard r's device."""
        _chk(self._lib.ukfb_group_gather_means(self._g, self._ptrs(out_devs)), "ukfb_group_gather_means")

    def last_gather_exchange(self) -> str:
        """which exchange the last gather_means used: "rccl" (one shard per device) or "copies" (shards sharing a device)"""
        return {0: "none", 1: "rccl", 2: "copies"}.get(int(self._lib.ukfb_group_last_gather_exchange(self._g)), "?")
