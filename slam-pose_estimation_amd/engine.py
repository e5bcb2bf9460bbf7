"""ctypes binding of the C-ABI in include/ukf_batch.h (lib/libukf_batch.so).

This is plumbing: every numeric operation happens in the HIP kernels behind the C-ABI.  There is no
CPU fallback -- if the shared library or a HIP device is missing, construction raises.

abi.py states the ABI (constants, structures, the type of every argument); load_library() declares it on the library, so
a call here passes plain Python values and ctypes converts, or refuses, each one by the header's type.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import abi
from .abi import *  # noqa: F401,F403  (the constants, the structures, SIGNATURES and EXPORTS stay reachable as engine.X)
from . import abi_relative
from .abi_relative import RELATIVE_NONE, RELATIVE_POSE, RELATIVE_POSITION, RELATIVE_ROTATION, RelativeIn, RelativeOut  # noqa: F401
from . import abi_robust
from .abi_robust import ROBUST_HUBER, ROBUST_MATCH, RobustOut, RobustRule  # noqa: F401
from . import abi_pda
from .abi_pda import PdaOut, PdaRule  # noqa: F401
from . import abi_assign
from .abi_assign import ASSIGN_BAD_SCENE, ASSIGN_COST_MAX, ASSIGN_MAX_TRACKS, ASSIGN_OK, AssignIn, AssignOut  # noqa: F401
from . import abi_jpda
from .abi_jpda import JPDA_BAD_SCENE, JPDA_LOG_RATIO_MAX, JPDA_MAX_TRACKS, JPDA_OK, JPDA_TOO_LARGE, JpdaIn, JpdaOut, WeightedOut  # noqa: F401
from . import abi_delayed_sensor
from .abi_delayed_sensor import DelayedSensorIn  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UKFB_LIB", os.path.join(_HERE, "lib", "libukf_batch.so"))  # UKFB_LIB: debug builds only


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
        abi.declare(lib)
        abi_relative.declare(lib)   # (include/ukf_batch_relative.h)
        abi_robust.declare(lib)     # (include/ukf_batch_robust.h)
        abi_delayed_sensor.declare(lib)   # (include/ukf_batch_delayed_sensor.h)
        abi_pda.declare(lib)        # (include/ukf_batch_pda.h)
        abi_assign.declare(lib)     # (include/ukf_batch_assign.h)
        abi_jpda.declare(lib)       # (include/ukf_batch_jpda.h)
        _lib = lib
    return _lib


def _invoke(lib, name: str, *args, what: Optional[str] = None):
    """Call the entry point `name` (`what` in the message, where that differs); an error code raises UkfbError."""
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.ukfb_last_error()
        raise UkfbError(f"{what or name} failed with code {rc}: {msg.decode() if msg else ''}")


def _typed_array(dtype):
    def array(a, shape=-1):
        return None if a is None else np.ascontiguousarray(a, dtype=dtype).reshape(shape)
    return array


# a contiguous NumPy array of that element type in that shape (flat unless given), None for None
_u8, _i32, _i64 = (_typed_array(t) for t in (np.uint8, np.int32, np.int64))


def _f64(a, shape=None):
    """The same for doubles, except that without a shape the array keeps its own."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def _typed_pointer(ctype):
    return lambda a: a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


# the ctypes pointer of a NumPy array of that element type, None for None: what a host-array argument of that type takes
_pd, _pi32, _pu32, _pu8, _pi64 = (_typed_pointer(t) for t in (C.c_double, C.c_int32, C.c_uint32, C.c_uint8, C.c_int64))


def _dev(x):
    """The device address behind an int, a torch tensor (data_ptr) or None, as a plain int or None: what a `void*` argument
    and a pointer field of a ctypes Structure take."""
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def _typed_dev(ctype):
    return lambda x: None if x is None else C.cast(_dev(x), C.POINTER(ctype))


# _dev as the typed pointer of a device array that the header types by its element (`const int32_t* meas_model_dev`)
_dev_d, _dev_i32, _dev_u32, _dev_u8, _dev_i64 = (_typed_dev(t) for t in (C.c_double, C.c_int32, C.c_uint32, C.c_uint8, C.c_int64))


def _int_or_i32(x, n):
    """An argument that is one int for the batch or an int32 array [n] -> (the int or 0, the array or None)."""
    if np.isscalar(x):
        return int(x), None
    return 0, _i32(x, n)


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
    return bool(load_library().ukfb_layout_supported(precision, lanes_per_filter))


def _dims(model: int, precision: int):
    """(S, D, PK, dtype): the state's scalars, its tangent dimension, the packed covariance's scalars, the device element type"""
    S, D = (13, 12) if model == MODEL_POSE else (14, 13)
    return S, D, D * (D + 1) // 2, np.float64 if precision == F64 else np.float32


# PoseUKF ctor defaults (PoseUKF.cpp:103-107)
_POSE_DEFAULT_NOISE = np.diag([0.01] * 3 + [0.001] * 3 + [0.00001] * 3 + [0.00001] * 3)


def _latch_orient_inputs(ukf, mu, first):
    """The OrientationUKF ctor's input latches (OrientationUKF.cpp:49-50) for the filters that `ukf` initialised from mu."""
    n = mu.shape[0]
    acc = np.zeros((n, 3)); acc[:, 2] = mu[:, 13]
    ukf.set_orient_inputs(gyro=np.zeros((n, 3)), acc=acc, first=first)


def _sensor_in(struct, model_dev, z_dev, Q_dev, q_is_uniform, mount_dev, mount, point_dev, point, **more):
    """ukfb_sensor_in, or ukfb_associate_in with the fields it has `more` of"""
    return struct(model_dev=_dev(model_dev), z_dev=_dev(z_dev), Q_dev=_dev(Q_dev), q_is_uniform=q_is_uniform,
                  mount_dev=_dev(mount_dev), mount_uniform=(C.c_double * 7)(*mount), point_dev=_dev(point_dev),
                  point_uniform=(C.c_double * 3)(*point), **more)


def _meas_outputs(n, m):
    """The results of a host update with an m-dimensional measurement, and their pointers in the order of the C-ABI."""
    o = {"z_pred": np.empty((n, m)), "S": np.empty((n, m, m)), "innov": np.empty((n, m)), "maha": np.empty(n),
         "loglik": np.empty(n), "status": np.empty(n, dtype=np.uint32)}
    return o, (_pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]), _pd(o["maha"]), _pd(o["loglik"]), _pu32(o["status"]))


def _process_events(ukf, fn: str, filter_index, ts_us, meas_model, z, Q):
    """ukfb_process_events and ukfb_group_process_events: one signature, one shape of arguments and results"""
    f = _i64(filter_index)
    n = f.size
    t, m = _i64(ts_us, n), _i32(meas_model, n)
    z = _f64(z, (n, 3)); Q = _f64(Q, (n, 3, 3))
    st, rounds = C.c_uint32(0), C.c_int64(0)
    ukf._call(fn, n, _pi64(f), _pi64(t), _pi32(m), _pd(z), _pd(Q), C.byref(st), C.byref(rounds))
    return int(st.value), int(rounds.value)


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
        kind = "given"
        if stream is None or stream == "torch":
            ts = _torch_current_stream(device)
            if ts is None and stream == "torch":
                raise UkfbError('stream="torch" needs torch with a visible GPU')
            kind = "torch" if ts is not None else "private"
            stream = ts if ts is not None else "private"
        if stream == "private":
            self.stream_kind, create, stream = "private", "ukfb_create", None
        else:
            self.stream_kind, create, stream = kind, "ukfb_create_on_stream", int(stream) or None
        _invoke(self._lib, create, C.byref(self._h), model, precision, capacity, device, stream)
        self.model, self.precision, self.capacity, self.device = model, precision, int(capacity), device
        self.S, self.D, self.PK, self.dtype = _dims(model, precision)
        if lanes_per_filter or cfg:
            self.configure(lanes_per_filter=lanes_per_filter, **cfg)

    def _call(self, name: str, *args, what: Optional[str] = None):
        """The entry point `name` on this engine's handle."""
        _invoke(self._lib, name, self._h, *args, what=what)

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
        self._call("ukfb_get_config", C.byref(c))
        return c

    def configure(self, **kw):
        c = self.config()
        for k, v in kw.items():
            if k == "lanes_per_filter" and not v:
                continue
            setattr(c, k, v)
        self._call("ukfb_set_config", C.byref(c))

    def sync(self):
        self._call("ukfb_sync")

    # ---- state
    def initialize(self, mu, cov, first: int = 0):
        mu = _f64(mu, (-1, self.S)); cov = _f64(cov, (-1, self.D, self.D))
        self._call("ukfb_initialize", first, mu.shape[0], _pd(mu), _pd(cov))

    def state(self, first: int = 0, count: Optional[int] = None, with_cov: bool = True):
        count = self.capacity - first if count is None else count
        mu = np.empty((count, self.S))
        cov = np.empty((count, self.D, self.D)) if with_cov else None
        init = np.empty(count, dtype=np.uint8)
        self._call("ukfb_get_state", first, count, _pd(mu), _pd(cov), _pu8(init))
        return (mu, cov, init.astype(bool)) if with_cov else (mu, init.astype(bool))

    def status(self, first: int = 0, count: Optional[int] = None):
        count = self.capacity - first if count is None else count
        st = np.empty(count, dtype=np.uint32)
        self._call("ukfb_get_status", first, count, _pu32(st))
        return st

    def status_summary(self) -> int:
        v = C.c_uint32(0)
        self._call("ukfb_get_status_summary", C.byref(v))
        return int(v.value)

    def set_last_measurement_time(self, t_us, first: int = 0):
        t = np.ascontiguousarray(t_us, dtype=np.int64)
        self._call("ukfb_set_last_measurement_time", first, t.size, _pi64(t), what="set_last_time")

    def last_measurement_time(self, first: int = 0, count: Optional[int] = None):
        count = self.capacity - first if count is None else count
        t = np.empty(count, dtype=np.int64)
        self._call("ukfb_get_last_measurement_time", first, count, _pi64(t), what="get_last_time")
        return t

    def device_views(self):
        mu, cov, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._call("ukfb_device_views", C.byref(mu), C.byref(cov), C.byref(st))
        return mu.value, cov.value, st.value

    # ---- noise / inputs
    def set_process_noise(self, R, first: Optional[int] = None):
        R = _f64(R)
        if R.ndim == 2:
            self._call("ukfb_set_process_noise", _pd(R))
        else:
            self._call("ukfb_set_process_noise_per_filter", first or 0, R.shape[0], _pd(R))

    def process_noise(self, filter_index: int = 0):
        R = np.empty((self.D, self.D))
        self._call("ukfb_get_process_noise", filter_index, _pd(R))
        return R

    def set_acceleration(self, acc_mu=None, acc_cov=None, first: int = 0):
        am, ac = _f64(acc_mu, (-1, 3)), _f64(acc_cov, (3, 3))
        self._call("ukfb_pose_set_acceleration", first, am.shape[0] if am is not None else 0, _pd(am), _pd(ac))

    def export_body_states(self, first: int = 0, count: Optional[int] = None):
        """BodyStateMeasurement::toRigidBodyState for a range of filters -> [count, 49] records."""
        count = self.capacity - first if count is None else count
        out = np.empty((count, BODY_STATE_SCALARS))
        self._call("ukfb_pose_export_body_states", first, count, _pd(out))
        return out

    def import_body_states(self, records, first: int = 0):
        """BodyStateMeasurement::fromRigidBodyState + initializeFilter from [count, 49] records."""
        rec = _f64(records, (-1, BODY_STATE_SCALARS))
        self._call("ukfb_pose_import_body_states", first, rec.shape[0], _pd(rec))

    def bind_acceleration_dev(self, acc_dev):
        self._call("ukfb_pose_bind_acceleration_dev", _dev(acc_dev))

    def set_orient_params(self, gyro_bias_tau: float, acc_bias_tau: float, earth_rotation):
        er = _f64(earth_rotation, (3,))
        self._call("ukfb_orient_set_params", gyro_bias_tau, acc_bias_tau, _pd(er))

    def set_orient_inputs(self, gyro=None, acc=None, first: int = 0):
        g, a = _f64(gyro, (-1, 3)), _f64(acc, (-1, 3))
        n = g.shape[0] if g is not None else (a.shape[0] if a is not None else 0)
        self._call("ukfb_orient_set_inputs", first, n, _pd(g), _pd(a))

    def bind_orient_inputs_dev(self, gyro_dev, acc_dev):
        self._call("ukfb_orient_bind_inputs_dev", _dev(gyro_dev), _dev(acc_dev))

    def rotation_rate(self, first: int = 0, count: Optional[int] = None):
        count = self.capacity - first if count is None else count
        out = np.empty((count, 3))
        self._call("ukfb_orient_get_rotation_rate", first, count, _pd(out))
        return out

    # ---- predict
    def predict(self, dt):
        if np.isscalar(dt):
            self._call("ukfb_predict", dt)
        else:
            d = _f64(dt, (self.capacity,))
            self._call("ukfb_predict_dt", _pd(d))

    def predict_timestamps(self, ts_us):
        t = _i64(ts_us, self.capacity)
        self._call("ukfb_predict_timestamps", _pi64(t))

    def predict_dt_dev(self, dt_dev):
        self._call("ukfb_predict_dt_dev", _dev_d(dt_dev))

    def predict_timestamps_dev(self, ts_dev):
        self._call("ukfb_predict_timestamps_dev", _dev_i64(ts_dev))

    # ---- update
    def update(self, meas_model, z, Q, active=None):
        z = _f64(z, (self.capacity, 3)); Q = _f64(Q, (self.capacity, 3, 3))
        if np.isscalar(meas_model):
            act = _u8(active)
            self._call("ukfb_update", int(meas_model), _pd(z), _pd(Q), _pu8(act))
        else:
            m = _i32(meas_model, self.capacity)
            self._call("ukfb_update_mixed", _pi32(m), _pd(z), _pd(Q))

    def update_dev(self, meas_model_uniform: int, z_dev, Q_dev, meas_model_dev=None):
        self._call("ukfb_update_dev", meas_model_uniform, _dev_i32(meas_model_dev), _dev(z_dev), _dev(Q_dev))

    # ---- innovation statistics and association (read-only: the engine's state and status are not touched)
    def innovation_dev(self, meas_model_uniform: int, candidates: int, z_dev, Q_dev, q_is_uniform: bool = False,
                       meas_model_dev=None, z_pred=None, S=None, innov=None, maha=None, loglik=None, best=None, status=None):
        """z_dev [candidates][capacity][3], Q_dev [capacity][9] (or 9 scalars with q_is_uniform); the keyword outputs are
        device buffers in engine precision (best int32, status uint32), None = not wanted.  Stream-ordered."""
        out = InnovationOut(_dev(z_pred), _dev(S), _dev(innov), _dev(maha), _dev(loglik), _dev(best), _dev(status))
        self._call("ukfb_innovation_dev", meas_model_uniform, _dev_i32(meas_model_dev), candidates, _dev(z_dev), _dev(Q_dev),
                   q_is_uniform, C.byref(out))

    def select_candidates_dev(self, candidates: int, best_dev, meas_model_uniform: int, z_dev, z_sel_dev, meas_model_sel_dev=None,
                              meas_model_dev=None):
        """z_sel[i] = z[best[i]][i], meas_model_sel[i] = -1 where best[i] < 0: update_dev(0, z_sel, Q, meas_model_sel) then
        applies the nearest gated candidate of every filter and leaves the others untouched."""
        self._call("ukfb_select_candidates_dev", candidates, _dev_i32(best_dev), meas_model_uniform, _dev_i32(meas_model_dev),
                   _dev(z_dev), _dev(z_sel_dev), _dev_i32(meas_model_sel_dev))

    def innovation(self, meas_model: int, z, Q):
        """Host arrays: z [candidates, capacity, 3] (or [capacity, 3] for one candidate), Q [capacity, 3, 3].  Returns a dict of
        NumPy arrays: z_pred [n, 4], S [n, 3, 3], innov [K, n, 3], maha [K, n], loglik [K, n], best [n], status [n]."""
        n = self.capacity
        z = _f64(z, (-1, n, 3)); Q = _f64(Q, (n, 3, 3))
        K = z.shape[0]
        o = {"z_pred": np.empty((n, 4)), "S": np.empty((n, 3, 3)), "innov": np.empty((K, n, 3)), "maha": np.empty((K, n)),
             "loglik": np.empty((K, n)), "best": np.empty(n, dtype=np.int32), "status": np.empty(n, dtype=np.uint32)}
        self._call("ukfb_innovation", int(meas_model), K, _pd(z), _pd(Q), _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]),
                   _pd(o["maha"]), _pd(o["loglik"]), _pi32(o["best"]), _pu32(o["status"]))
        return o

    # ---- filter banks: capacity / M tracks of M hypotheses, track-major (hypothesis j of track t = filter t * M + j)
    def bank_weights_dev(self, hypotheses: int, logw_in, loglik, logw_out, w_out=None, status=None):
        """logw_out = logw_in + loglik - logsumexp over a track's hypotheses, w_out = exp(logw_out).  Torch tensors (or device
        addresses) of [capacity] in engine precision; logw_in None = uniform, loglik None = normalise only; status uint32 [T]."""
        self._call("ukfb_bank_weights_dev", hypotheses, _dev(logw_in), _dev(loglik), _dev(logw_out), _dev(w_out), _dev_u32(status))

    def bank_combine_dev(self, hypotheses: int, w, mu_out, cov_packed_out=None, status=None):
        """Mixture moments of every track: w [capacity], mu_out [T, S], cov_packed_out [T, PK] (lower triangle).  Read-only."""
        self._call("ukfb_bank_combine_dev", hypotheses, _dev(w), _dev(mu_out), _dev(cov_packed_out), _dev_u32(status))

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
        self._call("ukfb_bank_mix_dev", hypotheses, _dev(w), _pd(P), _dev(w_pred), _dev_u32(status))
        return w_pred, status

    def bank_combine(self, hypotheses: int, w):
        """Host arrays: w [capacity] -> (mu [T, S], cov [T, D, D], status [T])"""
        w = _f64(w, (self.capacity,))
        T = self.capacity // max(int(hypotheses), 1)
        mu, cov, st = np.empty((T, self.S)), np.empty((T, self.D, self.D)), np.empty(T, dtype=np.uint32)
        self._call("ukfb_bank_combine", hypotheses, _pd(w), _pd(mu), _pd(cov), _pu32(st))
        return mu, cov, st

    def bank_mix(self, hypotheses: int, w, transition):
        """Host arrays: w [capacity], transition [M, M] -> (w_pred [capacity], status [T]); replaces mean and covariance"""
        w = _f64(w, (self.capacity,))
        P = _f64(transition, (hypotheses, hypotheses))
        T = self.capacity // max(int(hypotheses), 1)
        wp, st = np.empty(self.capacity), np.empty(T, dtype=np.uint32)
        self._call("ukfb_bank_mix", hypotheses, _pd(w), _pd(P), _pd(wp), _pu32(st))
        return wp, st

    # ---- fixed-interval smoothing: history rings [slots, capacity, S] / [slots, capacity, PK] in engine precision
    def history_push_dev(self, slots: int, slot: int, mu_hist, cov_hist):
        """Stream-ordered copy of the engine's current mean and packed covariance into slot `slot` of the caller's rings (torch
        tensors or device addresses); ordered behind every launch enqueued so far, split launches included.  No allocation."""
        self._call("ukfb_history_push_dev", slots, slot, _dev(mu_hist), _dev(cov_hist))

    def smooth_dev(self, dt, slots: int, first_slot: int, mu_hist, cov_hist, mu_out=None, cov_out=None, status=None,
                   in_a_dev=None, in_b_dev=None):
        """RTS backward pass over the window of len(dt) + 1 steps that starts at slot first_slot (step c in slot (first_slot + c)
        % slots); dt[c] (host) is the time step of the prediction c -> c + 1.  mu_out / cov_out: rings like the history, None =
        in place (pass cov_out=False for no covariance output); status uint32 / int32 [capacity] or None; in_a_dev / in_b_dev:
        input rings [slots, capacity, 3] or None (the latched inputs).  Caller-supplied buffers: nothing is allocated.
        Read-only on the engine.  Returns (mu_out, cov_out)."""
        d = _f64(dt, -1)
        mu_out = mu_hist if mu_out is None else mu_out
        cov_out = cov_hist if cov_out is None else (None if cov_out is False else cov_out)
        self._call("ukfb_smooth_dev", d.size + 1, _pd(d), slots, first_slot, _dev(mu_hist), _dev(cov_hist), _dev(in_a_dev),
                   _dev(in_b_dev), _dev(mu_out), _dev(cov_out), _dev_u32(status))
        return mu_out, cov_out

    def smooth(self, dt, mu, cov, in_a=None, in_b=None):
        """Host arrays in window order: mu [steps, capacity, S], cov [steps, capacity, D, D], dt [steps - 1], in_a / in_b
        [steps, capacity, 3] or None -> (mu_s, cov_s, status [capacity]); synchronises"""
        d = _f64(dt, -1)
        steps, n = d.size + 1, self.capacity
        mu = _f64(mu, (steps, n, self.S)).copy(); cov = _f64(cov, (steps, n, self.D, self.D)).copy()
        a, b = _f64(in_a, (steps, n, 3)), _f64(in_b, (steps, n, 3))
        st = np.zeros(n, dtype=np.uint32)
        self._call("ukfb_smooth", steps, _pd(d), _pd(mu), _pd(cov), _pd(a), _pd(b), _pu32(st))
        return mu, cov, st

    # ---- forecast: rings [slots, capacity, S] / [slots, capacity, PK] in engine precision, the history's format
    @staticmethod
    def _forecast_steps(dt, ts_us):
        if (dt is None) == (ts_us is None):
            raise UkfbError("forecast: exactly one of dt and ts_us")
        d, t = _f64(dt, -1), _i64(ts_us)
        return d, t, (d.size if d is not None else t.size)

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
        d, t, steps = self._forecast_steps(dt, ts_us)
        self._call("ukfb_forecast_dev", steps, _pd(d), _pi64(t), slots, first_slot, _dev(start_mu), _dev(start_cov), _dev(in_a_dev),
                   _dev(in_b_dev), _dev(mu_out), _dev(cov_out), _dev_u32(status))
        return mu_out, cov_out

    def forecast(self, dt=None, ts_us=None, start_mu=None, start_cov=None, in_a=None, in_b=None, with_cov: bool = True):
        """Host arrays in window order: dt or ts_us [steps], start_mu [capacity, S] and start_cov [capacity, D, D] (None: the
        engine's state), in_a / in_b [steps, capacity, 3] or None -> (mu [steps, capacity, S], cov [steps, capacity, D, D] or
        None, status [capacity]); synchronises"""
        d, t, steps = self._forecast_steps(dt, ts_us)
        n = self.capacity
        sm, sc = _f64(start_mu, (n, self.S)), _f64(start_cov, (n, self.D, self.D))
        a, b = _f64(in_a, (steps, n, 3)), _f64(in_b, (steps, n, 3))
        mu = np.zeros((steps, n, self.S))
        cov = np.zeros((steps, n, self.D, self.D)) if with_cov else None
        st = np.zeros(n, dtype=np.uint32)
        self._call("ukfb_forecast", steps, _pd(d), _pi64(t), _pd(sm), _pd(sc), _pd(a), _pd(b), _pd(mu), _pd(cov), _pu32(st))
        return mu, cov, st

    # ---- filter lifecycle: records [n, S] / [n, PK] / int64 [n] / uint8 [n] / [n, 3] / [n, 3] / [n, D, D] / uint32 [n] on the device
    @staticmethod
    def _records(mu, cov_packed, last_ts_us, initialised, in_a, in_b, noise, status):
        return FilterRecords(mu=_dev(mu), cov_packed=_dev(cov_packed), last_ts_us=_dev(last_ts_us), initialised=_dev(initialised),
                             in_a=_dev(in_a), in_b=_dev(in_b), noise=_dev(noise), status=_dev(status))

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
        self._call("ukfb_gather_filters_dev", n, _dev_i32(index_dev), C.byref(rec))

    def scatter_filters_dev(self, index_dev, mu, cov_packed, last_ts_us=None, initialised=None, in_a=None, in_b=None, noise=None,
                            status=None, n: Optional[int] = None):
        """initializeFilter from device records: filter index_dev[k] <- record k.  mu and cov_packed are required;
        initialised None = 1 (a 0 retires the filter), last_ts_us None = 0; in_a / in_b go into the engine's latches, noise into
        the filter's per-filter entry (the engine must already store its noise per filter).  Among the items that name one
        filter the lowest wins; every other one, and every index outside [0, capacity), gets ST_INACTIVE in status.
        Stream-ordered, no synchronisation."""
        n = self._items(index_dev, n, self.capacity)
        rec = self._records(mu, cov_packed, last_ts_us, initialised, in_a, in_b, noise, status)
        self._call("ukfb_scatter_filters_dev", n, _dev_i32(index_dev), C.byref(rec))

    def retire_dev(self, retire_mask_dev):
        """uint8 / bool [capacity] on the device: a non-zero byte clears the filter's initialised flag and last measurement time"""
        self._call("ukfb_retire_dev", _dev_u8(retire_mask_dev))

    def compact_dev(self, group: int = 1, new_index=None, old_index=None, live=None):
        """Move the live groups of `group` consecutive filters to the front, in place (include/ukf_batch.h, "filter
        lifecycle").  new_index / old_index int32 [capacity] and live int64 [1] on the device, each may be None.  Bound input
        buffers are not moved: permute them with old_index."""
        self._call("ukfb_compact_dev", group, _dev_i32(new_index), _dev_i32(old_index), _dev_i64(live))

    def gather_filters(self, index=None, n: Optional[int] = None):
        """Host form: index int32 [n] or None (item k is filter k) -> (mu [n, S], cov [n, D, D], last_ts_us [n],
        initialised bool [n]); synchronises"""
        idx = _i32(index)
        n = (idx.size if idx is not None else self.capacity) if n is None else n
        mu, cov = np.zeros((n, self.S)), np.zeros((n, self.D, self.D))
        ts, init = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint8)
        self._call("ukfb_gather_filters", n, _pi32(idx), _pd(mu), _pd(cov), _pi64(ts), _pu8(init))
        return mu, cov, ts, init.astype(bool)

    def scatter_filters(self, index, mu, cov, last_ts_us=None, initialised=None):
        """Host form: filter index[k] <- (mu[k], cov[k] full D x D, last_ts_us[k] or 0, initialised[k] or 1); returns the
        per-item status; synchronises"""
        mu = _f64(mu, (-1, self.S)); cov = _f64(cov, (-1, self.D, self.D))
        n = mu.shape[0]
        idx, ts, init = _i32(index), _i64(last_ts_us, n), _u8(initialised, n)
        if idx is not None and idx.size != n:
            raise UkfbError("scatter_filters: one index per record")
        st = np.zeros(n, dtype=np.uint32)
        self._call("ukfb_scatter_filters", n, _pi32(idx), _pd(mu), _pd(cov), _pi64(ts), _pu8(init), _pu32(st))
        return st

    def compact(self, group: int = 1):
        """Host form -> (new_index int32 [capacity], old_index int32 [capacity], live); synchronises"""
        new, old = np.zeros(self.capacity, dtype=np.int32), np.zeros(self.capacity, dtype=np.int32)
        live = C.c_int64(0)
        self._call("ukfb_compact", group, _pi32(new), _pi32(old), C.byref(live))
        return new, old, int(live.value)

    # ---- joint state-block measurements: z in the state's own layout [capacity, S], Qz the packed lower triangle [capacity, PK]
    def update_state_dev(self, block_mask: int, z_dev, Qz_packed_dev, block_mask_dev=None, state_inflation: float = 1.0,
                         meas_inflation: float = 1.0, commit: bool = True, maha=None, loglik=None, status=None):
        """ukfom's update with the blocks `block_mask` selects as ONE measurement with its full covariance (BLOCK_* constants;
        block_mask_dev int32 [capacity] = a mask per filter, <= 0: none).  A record of device_views, a history slot or
        bank_combine_dev is a valid (z_dev, Qz_packed_dev) as it lies.  The update runs on state_inflation * Sigma and
        meas_inflation * Qz (1 / w, 1 / (1 - w): covariance intersection).  commit=False is read-only: only the keyword
        outputs (device buffers [capacity] in engine precision, status uint32 / int32) are written.  Stream-ordered."""
        out = StateMeasOut(_dev(maha), _dev(loglik), _dev(status))
        self._call("ukfb_update_state_dev", int(block_mask), _dev_i32(block_mask_dev), _dev(z_dev), _dev(Qz_packed_dev),
                   state_inflation, meas_inflation, commit, C.byref(out))

    def update_state(self, block_mask, z, Qz, state_inflation: float = 1.0, meas_inflation: float = 1.0, commit: bool = True):
        """Host arrays: z [capacity, S], Qz [capacity, D, D]; block_mask an int or an int32 array [capacity].  Returns
        (maha [capacity], loglik [capacity], status [capacity]); synchronises"""
        n = self.capacity
        z = _f64(z, (n, self.S)); Qz = _f64(Qz, (n, self.D, self.D))
        mask, per = _int_or_i32(block_mask, n)
        maha, ll, st = np.empty(n), np.empty(n), np.empty(n, dtype=np.uint32)
        self._call("ukfb_update_state", mask, _pi32(per), _pd(z), _pd(Qz), state_inflation, meas_inflation, commit, _pd(maha),
                   _pd(ll), _pu32(st))
        return maha, ll, st

    def update_body_states(self, block_mask: int, records, active=None):
        """Pose engines: [capacity, 49] RigidBodyState records (the shape of export_body_states) integrated as measurements
        of the blocks `block_mask` selects; active uint8 [capacity] or None.  Synchronises."""
        rec = _f64(records, (self.capacity, BODY_STATE_SCALARS))
        act = _u8(active, self.capacity)
        self._call("ukfb_pose_update_body_states", int(block_mask), _pd(rec), _pu8(act))

    # ---- sensor-frame measurements: z [capacity, 3], Q [capacity, 9] (or 9 scalars), mount [capacity, 7], point [capacity, 3]
    def _update_sensor_frame_dev(self, fn: str, model, commit, sensor, outputs):
        """ukfb_update_sensor_dev and ukfb_update_bearing_dev: one signature; `sensor` the arguments of _sensor_in, `outputs`
        the device buffers in ukfb_sensor_out's order"""
        sin = _sensor_in(SensorIn, *sensor)
        out = SensorOut(*[_dev(x) for x in outputs])
        self._call(fn, int(model), C.byref(sin), commit, C.byref(out))

    def update_sensor_dev(self, model: int, z_dev, Q_dev, q_is_uniform: bool = False, model_dev=None, mount_dev=None,
                          mount=SENSOR_MOUNT_IDENTITY, point_dev=None, point=(0.0, 0.0, 0.0), commit: bool = True, z_pred=None,
                          S=None, innov=None, maha=None, loglik=None, status=None):
        """ukfom's update through a sensor-frame model (SENSOR_* constants; model_dev int32 [capacity] = an id per filter,
        negative: none).  mount = r[3] then qs[4] (x, y, z, w), point = b[3]: host values for the whole batch, or device
        arrays per filter (mount_dev / point_dev).  commit=False is read-only: only the keyword outputs (device buffers in
        engine precision, status uint32 / int32) are written.  Stream-ordered."""
        self._update_sensor_frame_dev("ukfb_update_sensor_dev", model, commit,
                                      (model_dev, z_dev, Q_dev, q_is_uniform, mount_dev, mount, point_dev, point),
                                      (z_pred, S, innov, maha, loglik, status))

    def _update_sensor_frame(self, fn: str, model, z, Q, mount, point, commit):
        """ukfb_update_sensor and ukfb_update_bearing: one signature, one shape of arguments and results"""
        n = self.capacity
        z = _f64(z, (n, 3)); Q = _f64(Q, (n, 3, 3))
        uniform, per = _int_or_i32(model, n)
        mp, mu_ = _per_or_uniform(mount, n, 7)
        pp, pu = _per_or_uniform(point, n, 3)
        o, outputs = _meas_outputs(n, 3)
        self._call(fn, uniform, _pi32(per), _pd(z), _pd(Q), _pd(mp), _pd(mu_), _pd(pp), _pd(pu), commit, *outputs)
        return o

    def update_sensor(self, model, z, Q, mount=SENSOR_MOUNT_IDENTITY, point=(0.0, 0.0, 0.0), commit: bool = True):
        """Host arrays: z [capacity, 3], Q [capacity, 3, 3]; model an int or an int32 array [capacity]; mount [7] or
        [capacity, 7], point [3] or [capacity, 3].  Returns a dict of NumPy arrays: z_pred [n, 3], S [n, 3, 3], innov [n, 3],
        maha [n], loglik [n], status [n]; synchronises"""
        return self._update_sensor_frame("ukfb_update_sensor", model, z, Q, mount, point, commit)

    # ---- the robust sensor-frame update: update_sensor's arguments and a rule (include/ukf_batch_robust.h)
    def update_robust_dev(self, model: int, z_dev, Q_dev, rule: RobustRule, q_is_uniform: bool = False, model_dev=None,
                          mount_dev=None, mount=SENSOR_MOUNT_IDENTITY, point_dev=None, point=(0.0, 0.0, 0.0), commit: bool = True,
                          z_pred=None, S=None, innov=None, maha0=None, maha=None, loglik=None, scale=None, iterations=None,
                          status=None):
        """update_sensor_dev with an outlying sample down-weighted, not rejected: a filter whose raw distance maha0 exceeds the
        rule's threshold (chi2_m1 / chi2_m3 by the model's m) updates with scale * Q, scale from the rule's mode (ROBUST_MATCH:
        d^2(scale) = c^2 by Newton, ROBUST_HUBER: sqrt(maha0 / c^2)), clamped to [1, scale_max]; the engine's gate acts on
        maha0.  Keyword outputs as for update_sensor_dev, and maha0, scale (engine precision), iterations (int32).
        Stream-ordered."""
        sin = _sensor_in(SensorIn, model_dev, z_dev, Q_dev, q_is_uniform, mount_dev, mount, point_dev, point)
        out = RobustOut(*[_dev(x) for x in (z_pred, S, innov, maha0, maha, loglik, scale, iterations, status)])
        self._call("ukfb_update_robust_dev", int(model), C.byref(sin), C.byref(rule), commit, C.byref(out))

    def update_robust(self, model, z, Q, rule: RobustRule, mount=SENSOR_MOUNT_IDENTITY, point=(0.0, 0.0, 0.0), commit: bool = True):
        """Host arrays, shaped as for update_sensor.  Returns its dict of NumPy arrays with maha0 [n], scale [n] and iterations
        [n] (int32) added; synchronises"""
        n = self.capacity
        z = _f64(z, (n, 3)); Q = _f64(Q, (n, 3, 3))
        uniform, per = _int_or_i32(model, n)
        mp, mu_ = _per_or_uniform(mount, n, 7)
        pp, pu = _per_or_uniform(point, n, 3)
        o = {"z_pred": np.empty((n, 3)), "S": np.empty((n, 3, 3)), "innov": np.empty((n, 3)), "maha0": np.empty(n), "maha": np.empty(n),
             "loglik": np.empty(n), "scale": np.empty(n), "iterations": np.empty(n, dtype=np.int32), "status": np.empty(n, dtype=np.uint32)}
        self._call("ukfb_update_robust", uniform, _pi32(per), _pd(z), _pd(Q), _pd(mp), _pd(mu_), _pd(pp), _pd(pu), C.byref(rule), commit,
                   _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]), _pd(o["maha0"]), _pd(o["maha"]), _pd(o["loglik"]), _pd(o["scale"]),
                   _pi32(o["iterations"]), _pu32(o["status"]))
        return o

    # ---- bearing measurements: z [capacity, 3] a direction, Q [capacity, 9] (or 9 scalars), mount [capacity, 7], point [capacity, 3]
    def update_bearing_dev(self, model: int, z_dev, Q_dev, q_is_uniform: bool = False, model_dev=None, mount_dev=None,
                           mount=SENSOR_MOUNT_IDENTITY, point_dev=None, point=(0.0, 0.0, 0.0), commit: bool = True, z_pred=None,
                           S=None, innov=None, maha=None, loglik=None, status=None):
        """ukfom's update with a direction on the sphere S^2 (BEARING_* constants; model_dev int32 [capacity] = an id per
        filter, negative: none).  z need not be normalised; Q is the 3 x 3 covariance of the direction noise in the sensor
        frame, of which the tangent part at the predicted direction enters.  mount, point, commit and the keyword outputs as
        for update_sensor_dev; z_pred is a unit vector, S = Sigma_z + P Q P (3 x 3, rank 2), innov the sphere logarithm.
        Stream-ordered."""
        self._update_sensor_frame_dev("ukfb_update_bearing_dev", model, commit,
                                      (model_dev, z_dev, Q_dev, q_is_uniform, mount_dev, mount, point_dev, point),
                                      (z_pred, S, innov, maha, loglik, status))

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
        ain = _sensor_in(AssociateIn, model_dev, z_dev, Q_dev, q_is_uniform, mount_dev, mount, point_dev, point,
                         candidates=int(candidates), point_per_candidate=point_per_candidate)
        out = AssociateOut(_dev(z_pred), _dev(S), _dev(innov), _dev(maha), _dev(loglik), _dev(best), _dev(n_gated), _dev(status))
        self._call("ukfb_associate_sensor_dev", int(model), C.byref(ain), commit, C.byref(out))

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
        self._call("ukfb_associate_sensor", uniform, _pi32(per), K, _pd(z), _pd(Q), _pd(mp), _pd(mu_), _pd(pp), _pd(pu),
                   point_per_candidate, commit, _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]), _pd(o["maha"]), _pd(o["loglik"]),
                   _pi32(o["best"]), _pi32(o["n_gated"]), _pu32(o["status"]))
        return o

    # ---- probabilistic data association: associate_sensor's shared-h arguments and a rule (include/ukf_batch_pda.h)
    def update_pda_dev(self, model: int, candidates: int, z_dev, Q_dev, rule: PdaRule, q_is_uniform: bool = False, model_dev=None,
                       mount_dev=None, mount=SENSOR_MOUNT_IDENTITY, point_dev=None, point=(0.0, 0.0, 0.0), commit: bool = True,
                       z_pred=None, S=None, innov=None, maha=None, loglik=None, beta=None, beta0=None, innov_comb=None, best=None,
                       n_gated=None, status=None):
        """associate_sensor_dev in shared-h mode whose update uses EVERY candidate inside the gate at its posterior association
        weight (PDAF): beta [candidates, capacity] the weights (0 outside the gate, NaN where not scored), beta0 [capacity] the
        weight of "none of them", innov_comb [capacity, 3] = sum beta_k nu_k; the covariance is widened by the spread of the
        weighted innovations.  rule: P_D, P_G and the clutter density for m = 1 / m = 3.  The other keyword outputs as for
        associate_sensor_dev with H = 1; best is the candidate of the largest weight.  commit=False is read-only.
        Stream-ordered."""
        ain = _sensor_in(AssociateIn, model_dev, z_dev, Q_dev, q_is_uniform, mount_dev, mount, point_dev, point,
                         candidates=int(candidates), point_per_candidate=False)
        out = PdaOut(*[_dev(x) for x in (z_pred, S, innov, maha, loglik, beta, beta0, innov_comb, best, n_gated, status)])
        self._call("ukfb_update_pda_dev", int(model), C.byref(ain), C.byref(rule), commit, C.byref(out))

    def update_pda(self, model, z, Q, rule: PdaRule, mount=SENSOR_MOUNT_IDENTITY, point=(0.0, 0.0, 0.0), commit: bool = True):
        """Host arrays, shaped as for associate_sensor in shared-h mode: z [candidates, capacity, 3], point [3] or [capacity, 3].
        Returns a dict of NumPy arrays: z_pred [n, 3], S [n, 3, 3], innov [K, n, 3], maha / loglik / beta [K, n], beta0 [n],
        innov_comb [n, 3], best / n_gated / status [n]; synchronises"""
        n = self.capacity
        z = _f64(z)
        K = int(z.shape[0]) if z.ndim == 3 else 0
        z = _f64(z, (K, n, 3)); Q = _f64(Q, (n, 3, 3))
        uniform, per = _int_or_i32(model, n)
        mp, mu_ = _per_or_uniform(mount, n, 7)
        pp, pu = _per_or_uniform(point, n, 3)
        o = {"z_pred": np.empty((n, 3)), "S": np.empty((n, 3, 3)), "innov": np.empty((K, n, 3)), "maha": np.empty((K, n)),
             "loglik": np.empty((K, n)), "beta": np.empty((K, n)), "beta0": np.empty(n), "innov_comb": np.empty((n, 3)),
             "best": np.empty(n, dtype=np.int32), "n_gated": np.empty(n, dtype=np.int32), "status": np.empty(n, dtype=np.uint32)}
        self._call("ukfb_update_pda", uniform, _pi32(per), K, _pd(z), _pd(Q), _pd(mp), _pd(mu_), _pd(pp), _pd(pu), C.byref(rule), commit,
                   _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]), _pd(o["maha"]), _pd(o["loglik"]), _pd(o["beta"]), _pd(o["beta0"]),
                   _pd(o["innov_comb"]), _pi32(o["best"]), _pi32(o["n_gated"]), _pu32(o["status"]))
        return o

    # ---- global nearest-neighbour assignment across the filters of a scene (include/ukf_batch_assign.h)
    def assign_scenes_dev(self, candidates: int, cost_dev, scenes: int, scene_start_dev=None, tracks_per_scene: int = 0,
                          gate: float = -1.0, miss_dev=None, miss: float = 0.0, assign=None, owner=None, objective=None,
                          scene_status=None):
        """The one-to-one assignment of `candidates` detections to the filters of each of `scenes` scenes, contiguous runs of
        slots that share one detection list: scene_start_dev int32 [scenes + 1], or uniform scenes of tracks_per_scene slots.
        cost_dev [candidates, capacity] in engine precision (the maha or -2 loglik an association call wrote); pairs with a
        non-finite cost or, with gate >= 0, a cost above the gate are forbidden; miss_dev [capacity] (or the host value
        `miss`) is the cost of leaving a track without a detection, a non-finite entry takes the track out.  Keyword outputs
        (device buffers): assign int32 [capacity] (a drop-in for `best`), owner int32 [scenes, candidates], objective float64
        [scenes], scene_status uint32 [scenes].  Read-only on the filters.  Stream-ordered."""
        ain = AssignIn(_dev(cost_dev), int(candidates), int(scenes), _dev(scene_start_dev), int(tracks_per_scene), float(gate),
                       _dev(miss_dev), float(miss))
        out = AssignOut(_dev(assign), _dev(owner), _dev(objective), _dev(scene_status))
        self._call("ukfb_assign_scenes_dev", C.byref(ain), C.byref(out))

    def assign_scenes(self, cost, scene_start=None, tracks_per_scene: int = 0, gate: float = -1.0, miss=0.0, scenes=None):
        """Host arrays: cost [candidates, capacity]; scene_start int32 [scenes + 1], or uniform scenes of tracks_per_scene
        slots (`scenes` of them; default: all that fit); miss a float or an array [capacity].  Returns a dict of NumPy arrays:
        assign [n] (-1 where no scene covers a slot), owner [scenes, K], objective [scenes], scene_status [scenes];
        synchronises"""
        n = self.capacity
        cost = _f64(cost)
        K = int(cost.shape[0]) if cost.ndim == 2 else 0
        cost = _f64(cost, (K, n))
        start = _i32(scene_start)
        if scenes is None:
            scenes = len(start) - 1 if start is not None else (-(-n // tracks_per_scene) if tracks_per_scene > 0 else 0)
        miss_per, miss_uniform = (None, float(miss)) if np.isscalar(miss) else (_f64(miss, n), 0.0)
        ns = max(int(scenes), 0)
        o = {"assign": np.empty(n, dtype=np.int32), "owner": np.empty((ns, K), dtype=np.int32), "objective": np.empty(ns),
             "scene_status": np.empty(ns, dtype=np.uint32)}
        self._call("ukfb_assign_scenes", K, _pd(cost), int(scenes), _pi32(start), int(tracks_per_scene), float(gate), _pd(miss_per),
                   miss_uniform, _pi32(o["assign"]), _pi32(o["owner"]), _pd(o["objective"]), _pu32(o["scene_status"]))
        return o

    # ---- joint probabilistic data association: the marginals of a scene, the update with given weights (include/ukf_batch_jpda.h)
    def jpda_scenes_dev(self, candidates: int, loglik_dev, rule: PdaRule, scenes: int, scene_start_dev=None, tracks_per_scene: int = 0,
                        maha_dev=None, gate: float = -1.0, model: int = 0, model_dev=None, beta=None, beta0=None, free=None,
                        log_z=None, scene_status=None):
        """The exact joint association marginals of each of `scenes` scenes (at most 6 tracks each), contiguous runs of slots
        that share one detection list: scene_start_dev int32 [scenes + 1], or uniform scenes of tracks_per_scene slots.
        loglik_dev (and maha_dev, needed with gate >= 0) [candidates, capacity] in engine precision, as update_pda_dev or an
        association call wrote them; model / model_dev the sensor model of the tracks.  Keyword outputs (device buffers): beta
        [candidates, capacity] and beta0 [capacity] in engine precision -- they may be the arrays update_pda_dev filled: bad and
        too-large scenes and uncovered slots keep what is there --, free float64 [scenes, candidates], log_z float64 [scenes],
        scene_status uint32 [scenes].  Read-only on the filters.  Stream-ordered."""
        jin = JpdaIn(_dev(loglik_dev), _dev(maha_dev), int(candidates), int(scenes), _dev(scene_start_dev), int(tracks_per_scene),
                     float(gate), int(model), _dev(model_dev))
        out = JpdaOut(_dev(beta), _dev(beta0), _dev(free), _dev(log_z), _dev(scene_status))
        self._call("ukfb_jpda_scenes_dev", C.byref(jin), C.byref(rule), C.byref(out))

    def jpda_scenes(self, loglik, rule: PdaRule, scene_start=None, tracks_per_scene: int = 0, maha=None, gate: float = -1.0, model=0,
                    scenes=None):
        """Host arrays: loglik (and maha) [candidates, capacity]; scene_start int32 [scenes + 1], or uniform scenes of
        tracks_per_scene slots (`scenes` of them; default: all that fit); model an id or an int32 array [capacity].  Returns a
        dict of NumPy arrays: beta [K, n] and beta0 [n] (NaN where no good scene covers a slot), free [scenes, K], log_z
        [scenes], scene_status [scenes]; synchronises"""
        n = self.capacity
        loglik = _f64(loglik)
        K = int(loglik.shape[0]) if loglik.ndim == 2 else 0
        loglik = _f64(loglik, (K, n))
        maha = None if maha is None else _f64(maha, (K, n))
        start = _i32(scene_start)
        if scenes is None:
            scenes = len(start) - 1 if start is not None else (-(-n // tracks_per_scene) if tracks_per_scene > 0 else 0)
        uniform, per = _int_or_i32(model, n)
        ns = max(int(scenes), 0)
        o = {"beta": np.empty((K, n)), "beta0": np.empty(n), "free": np.empty((ns, K)), "log_z": np.empty(ns),
             "scene_status": np.empty(ns, dtype=np.uint32)}
        self._call("ukfb_jpda_scenes", K, _pd(loglik), _pd(maha), int(scenes), _pi32(start), int(tracks_per_scene), float(gate), uniform,
                   _pi32(per), C.byref(rule), _pd(o["beta"]), _pd(o["beta0"]), _pd(o["free"]), _pd(o["log_z"]), _pu32(o["scene_status"]))
        return o

    def update_weighted_dev(self, model: int, candidates: int, z_dev, Q_dev, weight_dev, q_is_uniform: bool = False, model_dev=None,
                            mount_dev=None, mount=SENSOR_MOUNT_IDENTITY, point_dev=None, point=(0.0, 0.0, 0.0), commit: bool = True,
                            z_pred=None, S=None, innov=None, maha=None, loglik=None, weight_used=None, beta0=None, innov_comb=None,
                            n_used=None, status=None):
        """update_pda_dev whose association weights are READ from weight_dev [candidates, capacity] (engine precision) instead
        of computed: the joint marginals jpda_scenes_dev wrote, or any weights the caller normalised.  A weight counts where
        its candidate is scored with a finite d^2 and the weight is finite and > 0; the weights are used as w / max(1, sum w)
        (weight_used), beta0 = 1 - sum of them; cfg.gate_chi2 plays no part.  The other keyword outputs as for
        update_pda_dev; n_used int32 [capacity].  commit=False is read-only.  Stream-ordered."""
        ain = _sensor_in(AssociateIn, model_dev, z_dev, Q_dev, q_is_uniform, mount_dev, mount, point_dev, point,
                         candidates=int(candidates), point_per_candidate=False)
        out = WeightedOut(*[_dev(x) for x in (z_pred, S, innov, maha, loglik, weight_used, beta0, innov_comb, n_used, status)])
        self._call("ukfb_update_weighted_dev", int(model), C.byref(ain), _dev(weight_dev), commit, C.byref(out))

    def update_weighted(self, model, z, Q, weight, mount=SENSOR_MOUNT_IDENTITY, point=(0.0, 0.0, 0.0), commit: bool = True):
        """Host arrays, shaped as for update_pda: z [candidates, capacity, 3], weight [candidates, capacity].  Returns a dict of
        NumPy arrays: z_pred [n, 3], S [n, 3, 3], innov [K, n, 3], maha / loglik / weight_used [K, n], beta0 [n], innov_comb
        [n, 3], n_used / status [n]; synchronises"""
        n = self.capacity
        z = _f64(z)
        K = int(z.shape[0]) if z.ndim == 3 else 0
        z = _f64(z, (K, n, 3)); Q = _f64(Q, (n, 3, 3)); weight = _f64(weight, (K, n))
        uniform, per = _int_or_i32(model, n)
        mp, mu_ = _per_or_uniform(mount, n, 7)
        pp, pu = _per_or_uniform(point, n, 3)
        o = {"z_pred": np.empty((n, 3)), "S": np.empty((n, 3, 3)), "innov": np.empty((K, n, 3)), "maha": np.empty((K, n)),
             "loglik": np.empty((K, n)), "weight_used": np.empty((K, n)), "beta0": np.empty(n), "innov_comb": np.empty((n, 3)),
             "n_used": np.empty(n, dtype=np.int32), "status": np.empty(n, dtype=np.uint32)}
        self._call("ukfb_update_weighted", uniform, _pi32(per), K, _pd(z), _pd(Q), _pd(mp), _pd(mu_), _pd(pp), _pd(pu), _pd(weight), commit,
                   _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]), _pd(o["maha"]), _pd(o["loglik"]), _pd(o["weight_used"]), _pd(o["beta0"]),
                   _pd(o["innov_comb"]), _pi32(o["n_used"]), _pu32(o["status"]))
        return o

    # ---- user-defined measurement models: X [capacity, 2 D + 1, S], delta [capacity, 2 D + 1, D], Z [capacity, 2 D + 1, m]
    def sigma_points_dev(self, X_out=None, delta_out=None, status=None):
        """The sigma points of every filter into device buffers in engine precision, filter-major: X_out [capacity, 2 D + 1, S]
        (point 0 = mu, 1 + 2 j = mu (+) L col j, 2 + 2 j = mu (+) (-L col j)), delta_out [capacity, 2 D + 1, D] the tangent
        offsets themselves; either may be None, not both.  status uint32 / int32 [capacity] or None: 0, ST_UNINITIALISED or
        ST_ERR_CHOLESKY (rows of NaN).  Read-only on the engine.  Stream-ordered."""
        self._call("ukfb_sigma_points_dev", _dev(X_out), _dev(delta_out), _dev_u32(status))

    def update_sampled_dev(self, m: int, Z_dev, z_dev, Q_dev, q_is_uniform: bool = False, active_dev=None, commit: bool = True,
                           z_pred=None, S=None, innov=None, maha=None, loglik=None, status=None):
        """ukfom's update finished from the caller's samples Z_dev [capacity, 2 D + 1, m] = h(X) of sigma_points_dev's X
        (m = 1 ... SAMPLED_MAX_M); z_dev [capacity, m], Q_dev [capacity, m, m] (one m x m with q_is_uniform), active_dev uint8
        [capacity] or None.  The state must not change between the export and this call.  z and Z may be written relative to
        any per-filter origin (fp32 engines: one near the values).  commit=False is read-only: only the keyword outputs
        (device buffers in engine precision, status uint32 / int32) are written.  Stream-ordered."""
        sin = SampledIn(int(m), _dev(Z_dev), _dev(z_dev), _dev(Q_dev), q_is_uniform, _dev(active_dev))
        out = SampledOut(_dev(z_pred), _dev(S), _dev(innov), _dev(maha), _dev(loglik), _dev(status))
        self._call("ukfb_update_sampled_dev", C.byref(sin), commit, C.byref(out))

    def sigma_points(self):
        """Host form -> (X [capacity, 2 D + 1, S], delta [capacity, 2 D + 1, D], status [capacity]); synchronises"""
        n, pts = self.capacity, 2 * self.D + 1
        X, delta, st = np.empty((n, pts, self.S)), np.empty((n, pts, self.D)), np.empty(n, dtype=np.uint32)
        self._call("ukfb_sigma_points", _pd(X), _pd(delta), _pu32(st))
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
        act = _u8(active, n)
        o, outputs = _meas_outputs(n, m)
        self._call("ukfb_update_sampled", m, _pd(Z), _pd(z), _pd(Q), uniform, _pu8(act), commit, *outputs)
        return o

    # ---- user-defined process models: XX [capacity, 2 D + 1, S] = f(X) of sigma_points_dev's X, R [capacity, D, D]
    def predict_sampled_dev(self, XX, R, r_is_uniform: bool = False, active_dev=None, commit: bool = True, mu=None,
                            cov_packed=None, status=None):
        """ukfom's predict finished from the caller's propagated sigma points XX [capacity, 2 D + 1, S] = f(X) of
        sigma_points_dev's X and the caller's R [capacity, D, D] (one D x D with r_is_uniform; taken as given, the lower triangle
        is read); active_dev uint8 [capacity] or None.  Times, noise tables and latches are not touched.  commit=False is
        read-only: only the keyword outputs (device buffers in engine precision: mu [capacity, S], cov_packed [capacity, PK];
        status uint32 / int32) are written.  Stream-ordered, nothing is allocated."""
        pin = PredictSampledIn(_dev(XX), _dev(R), r_is_uniform, _dev(active_dev))
        out = PredictSampledOut(_dev(mu), _dev(cov_packed), _dev(status))
        self._call("ukfb_predict_sampled_dev", C.byref(pin), commit, C.byref(out))

    def predict_sampled(self, XX, R, active=None, commit: bool = True):
        """Host arrays: XX [capacity, 2 D + 1, S], R [capacity, D, D] or [D, D] (one for the batch); active uint8 [capacity] or
        None.  Returns a dict of NumPy arrays: mu [n, S], cov [n, D, D], status [n]; synchronises"""
        n, pts, S, D = self.capacity, 2 * self.D + 1, self.S, self.D
        XX = _f64(XX, (n, pts, S)); R = _f64(R)
        uniform = R.ndim == 2
        R = R.reshape(D, D) if uniform else R.reshape(n, D, D)
        act = _u8(active, n)
        o = {"mu": np.empty((n, S)), "cov": np.empty((n, D, D)), "status": np.empty(n, dtype=np.uint32)}
        self._call("ukfb_predict_sampled", _pd(XX), _pd(R), uniform, _pu8(act), commit, _pd(o["mu"]), _pd(o["cov"]), _pu32(o["status"]))
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
        cin = ConditionIn(_dev(var_floor_dev), float(eig_floor), _dev(select_dev), renormalize_quaternion)
        out = ConditionOut(_dev(eig_min), _dev(eig_max), _dev(mu), _dev(cov_packed), _dev(status))
        self._call("ukfb_condition_dev", C.byref(cin), commit, C.byref(out))

    def condition(self, var_floor, eig_floor: float, select=None, renormalize_quaternion: bool = False, commit: bool = True):
        """Host arrays: var_floor [D] (every entry finite and > 0), select uint8 [capacity] or None.  Returns a dict of NumPy
        arrays: eig_min [n], eig_max [n], mu [n, S], cov [n, D, D], status [n]; synchronises"""
        n, S, D = self.capacity, self.S, self.D
        v = _f64(var_floor, (D,))
        sel = _u8(select, n)
        o = {"eig_min": np.empty(n), "eig_max": np.empty(n), "mu": np.empty((n, S)), "cov": np.empty((n, D, D)),
             "status": np.empty(n, dtype=np.uint32)}
        self._call("ukfb_condition", _pd(v), eig_floor, _pu8(sel), renormalize_quaternion, commit, _pd(o["eig_min"]),
                   _pd(o["eig_max"]), _pd(o["mu"]), _pd(o["cov"]), _pu32(o["status"]))
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
        d = _f64(dt, -1)
        per = lambda x: (0, _dev(x)) if hasattr(x, "data_ptr") else (int(x), None)
        (lag_u, lag_p), (mod_u, mod_p) = per(lag), per(meas_model)
        din = DelayedIn(d.size + 1, _pd(d) if d.size else None, int(slots), int(first_slot), _dev(mu_hist), _dev(cov_hist),
                        _dev(in_a_dev), _dev(in_b_dev), lag_u, lag_p, mod_u, mod_p, _dev(z_dev), _dev(Q_dev), q_is_uniform)
        out = DelayedOut(_dev(z_pred), _dev(S), _dev(innov), _dev(maha), _dev(loglik), _dev(status), _dev(mu_out), _dev(cov_out))
        self._call("ukfb_update_delayed_dev", C.byref(din), commit, C.byref(out))

    def update_delayed(self, dt, mu_hist, cov_hist, lag, meas_model, z, Q, in_a=None, in_b=None, commit: bool = True):
        """Host arrays in window order: mu_hist [steps, capacity, S], cov_hist [steps, capacity, D, D] (the last step is not
        read), dt [steps - 1], in_a / in_b [steps, capacity, 3] or None; lag / meas_model an int or an int32 array [capacity];
        z [capacity, 3], Q [capacity, 3, 3].  Returns a dict of NumPy arrays: z_pred [n, 4], S [n, 3, 3], innov [n, 3], maha,
        loglik, status [n], mu_out [n, S], cov_out [n, D, D]; synchronises"""
        d = _f64(dt, -1)
        steps, n = d.size + 1, self.capacity
        mu_hist = _f64(mu_hist, (steps, n, self.S)); cov_hist = _f64(cov_hist, (steps, n, self.D, self.D))
        a, b = _f64(in_a, (steps, n, 3)), _f64(in_b, (steps, n, 3))
        z = _f64(z, (n, 3)); Q = _f64(Q, (n, 3, 3))
        (lag_u, lag_p), (mod_u, mod_p) = _int_or_i32(lag, n), _int_or_i32(meas_model, n)
        o = {"z_pred": np.empty((n, 4)), "S": np.empty((n, 3, 3)), "innov": np.empty((n, 3)), "maha": np.empty(n),
             "loglik": np.empty(n), "status": np.empty(n, dtype=np.uint32), "mu_out": np.empty((n, self.S)),
             "cov_out": np.empty((n, self.D, self.D))}
        self._call("ukfb_update_delayed", steps, _pd(d) if d.size else None, _pd(mu_hist), _pd(cov_hist), _pd(a), _pd(b), lag_u,
                   _pi32(lag_p), mod_u, _pi32(mod_p), _pd(z), _pd(Q), commit, _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]),
                   _pd(o["maha"]), _pd(o["loglik"]), _pu32(o["status"]), _pd(o["mu_out"]), _pd(o["cov_out"]))
        return o

    def delayed_lag_dev(self, step_ts_us, sample_ts_us_dev, lag_out_dev):
        """step_ts_us: host int64 stamps of the window's steps (strictly increasing); sample_ts_us_dev int64 [capacity] ->
        lag_out_dev int32 [capacity]: the step nearest each sample (ties: the older), 0 for a sample newer than the present,
        len(step_ts_us) (out of the window) for one older than the first step by more than half a step.  Stream-ordered."""
        ts = _i64(step_ts_us)
        self._call("ukfb_delayed_lag_dev", ts.size, _pi64(ts), _dev_i64(sample_ts_us_dev), _dev_i32(lag_out_dev))

    # ---- relative measurements: an increment between a step of the delayed update's window and the present (Pose engines)
    def update_relative_dev(self, dt, slots: int, first_slot: int, mu_hist, cov_hist, lag, model, z_dev, Q_dev,
                            q_is_uniform: bool = False, in_a_dev=None, in_b_dev=None, commit: bool = True, z_pred=None, S=None,
                            innov=None, maha=None, loglik=None, status=None, mu_out=None, cov_out=None):
        """An increment "since step n - lag you moved by dp and turned by dq" corrects the current state through the history
        ring (include/ukf_batch_relative.h): the update on the pair (present, clone of that step).  The window
        is update_delayed_dev's.  lag / model (RELATIVE_POSE / RELATIVE_POSITION / RELATIVE_ROTATION): an int for the whole batch
        or an int32 device array [capacity]; a lag <= 0 is INACTIVE.  z_dev [capacity, 7] (dp, then dq as x y z w), Q_dev
        [capacity, 36] (36 scalars with q_is_uniform), tangent order (dp, dtheta).  commit=False is read-only: only the keyword
        outputs (z_pred [capacity, 7], S [capacity, 36], innov [capacity, 6], maha, loglik, status, mu_out [capacity, S],
        cov_out [capacity, PK]) are written.  Stream-ordered, nothing is allocated."""
        d = _f64(dt, -1)
        per = lambda x: (0, _dev(x)) if hasattr(x, "data_ptr") else (int(x), None)
        (lag_u, lag_p), (mod_u, mod_p) = per(lag), per(model)
        rin = RelativeIn(d.size + 1, _pd(d) if d.size else None, int(slots), int(first_slot), _dev(mu_hist), _dev(cov_hist),
                         _dev(in_a_dev), _dev(in_b_dev), lag_u, lag_p, mod_u, mod_p, _dev(z_dev), _dev(Q_dev), q_is_uniform)
        out = RelativeOut(_dev(z_pred), _dev(S), _dev(innov), _dev(maha), _dev(loglik), _dev(status), _dev(mu_out), _dev(cov_out))
        self._call("ukfb_update_relative_dev", C.byref(rin), commit, C.byref(out))

    def update_relative(self, dt, mu_hist, cov_hist, lag, model, z, Q, in_a=None, in_b=None, commit: bool = True):
        """Host arrays in window order, as update_delayed: mu_hist [steps, capacity, S], cov_hist [steps, capacity, D, D] (the
        last step is not read), dt [steps - 1], in_a / in_b [steps, capacity, 3] or None; lag / model an int or an int32 array
        [capacity]; z [capacity, 7], Q [capacity, 6, 6].  Returns a dict of NumPy arrays: z_pred [n, 7], S [n, 6, 6], innov
        [n, 6], maha, loglik, status [n], mu_out [n, S], cov_out [n, D, D]; synchronises"""
        d = _f64(dt, -1)
        steps, n = d.size + 1, self.capacity
        mu_hist = _f64(mu_hist, (steps, n, self.S)); cov_hist = _f64(cov_hist, (steps, n, self.D, self.D))
        a, b = _f64(in_a, (steps, n, 3)), _f64(in_b, (steps, n, 3))
        z = _f64(z, (n, 7)); Q = _f64(Q, (n, 6, 6))
        (lag_u, lag_p), (mod_u, mod_p) = _int_or_i32(lag, n), _int_or_i32(model, n)
        o = {"z_pred": np.empty((n, 7)), "S": np.empty((n, 6, 6)), "innov": np.empty((n, 6)), "maha": np.empty(n),
             "loglik": np.empty(n), "status": np.empty(n, dtype=np.uint32), "mu_out": np.empty((n, self.S)),
             "cov_out": np.empty((n, self.D, self.D))}
        self._call("ukfb_update_relative", steps, _pd(d) if d.size else None, _pd(mu_hist), _pd(cov_hist), _pd(a), _pd(b), lag_u,
                   _pi32(lag_p), mod_u, _pi32(mod_p), _pd(z), _pd(Q), commit, _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]),
                   _pd(o["maha"]), _pd(o["loglik"]), _pu32(o["status"]), _pd(o["mu_out"]), _pd(o["cov_out"]))
        return o

    # ---- late sensor-frame samples: update_delayed's window with update_sensor's models and inputs
    def update_delayed_sensor_dev(self, dt, slots: int, first_slot: int, mu_hist, cov_hist, lag, model, z_dev, Q_dev,
                                  q_is_uniform: bool = False, mount_dev=None, mount=SENSOR_MOUNT_IDENTITY, point_dev=None,
                                  point=(0.0, 0.0, 0.0), rate_dev=None, in_a_dev=None, in_b_dev=None, commit: bool = True,
                                  z_pred=None, S=None, innov=None, maha=None, loglik=None, status=None, mu_out=None, cov_out=None):
        """A sensor-frame sample (SENSOR_* constants: a lever-arm fix, range, landmark sighting ...) taken `lag` steps ago corrects
        the current state through the history ring (include/ukf_batch_delayed_sensor.h): update_delayed_dev with the h of
        update_sensor_dev, evaluated on the smoothed state of the sample's own step.  The window is update_delayed_dev's.  lag /
        model: an int for the whole batch or an int32 device array [capacity].  z_dev [capacity, 3], Q_dev [capacity, 9] (9
        scalars with q_is_uniform); mount = r[3] then qs[4] (x, y, z, w), point = b[3]: host values for the whole batch, or
        device arrays per filter (mount_dev / point_dev).  rate_dev [capacity, 3]: the rotation rate at the time of the sample
        (SENSOR_ORIENT_VELOCITY); None: the rotation-rate ring in_b_dev at the sample's step when it is given and lag >= 1, else
        the engine's latch.  commit=False is read-only: only the keyword outputs (update_delayed_dev's) are written.
        Stream-ordered, nothing is allocated."""
        d = _f64(dt, -1)
        per = lambda x: (0, _dev(x)) if hasattr(x, "data_ptr") else (int(x), None)
        (lag_u, lag_p), (mod_u, mod_p) = per(lag), per(model)
        din = DelayedSensorIn(d.size + 1, _pd(d) if d.size else None, int(slots), int(first_slot), _dev(mu_hist), _dev(cov_hist),
                              _dev(in_a_dev), _dev(in_b_dev), lag_u, lag_p, mod_u, mod_p, _dev(z_dev), _dev(Q_dev), q_is_uniform,
                              _dev(mount_dev), (C.c_double * 7)(*mount), _dev(point_dev), (C.c_double * 3)(*point), _dev(rate_dev))
        out = DelayedOut(_dev(z_pred), _dev(S), _dev(innov), _dev(maha), _dev(loglik), _dev(status), _dev(mu_out), _dev(cov_out))
        self._call("ukfb_update_delayed_sensor_dev", C.byref(din), commit, C.byref(out))

    def update_delayed_sensor(self, dt, mu_hist, cov_hist, lag, model, z, Q, mount=SENSOR_MOUNT_IDENTITY, point=(0.0, 0.0, 0.0),
                              rate=None, in_a=None, in_b=None, commit: bool = True):
        """Host arrays in window order, as update_delayed: mu_hist [steps, capacity, S], cov_hist [steps, capacity, D, D] (the
        last step is not read), dt [steps - 1], in_a / in_b [steps, capacity, 3] or None; lag / model an int or an int32 array
        [capacity]; z [capacity, 3], Q [capacity, 3, 3]; mount [7] or [capacity, 7], point [3] or [capacity, 3]; rate
        [capacity, 3] or None.  Returns update_delayed's dict of NumPy arrays; synchronises"""
        d = _f64(dt, -1)
        steps, n = d.size + 1, self.capacity
        mu_hist = _f64(mu_hist, (steps, n, self.S)); cov_hist = _f64(cov_hist, (steps, n, self.D, self.D))
        a, b = _f64(in_a, (steps, n, 3)), _f64(in_b, (steps, n, 3))
        z = _f64(z, (n, 3)); Q = _f64(Q, (n, 3, 3))
        (lag_u, lag_p), (mod_u, mod_p) = _int_or_i32(lag, n), _int_or_i32(model, n)
        mp, mu_ = _per_or_uniform(mount, n, 7)
        pp, pu = _per_or_uniform(point, n, 3)
        w = _f64(rate, (n, 3))
        o = {"z_pred": np.empty((n, 4)), "S": np.empty((n, 3, 3)), "innov": np.empty((n, 3)), "maha": np.empty(n),
             "loglik": np.empty(n), "status": np.empty(n, dtype=np.uint32), "mu_out": np.empty((n, self.S)),
             "cov_out": np.empty((n, self.D, self.D))}
        self._call("ukfb_update_delayed_sensor", steps, _pd(d) if d.size else None, _pd(mu_hist), _pd(cov_hist), _pd(a), _pd(b),
                   lag_u, _pi32(lag_p), mod_u, _pi32(mod_p), _pd(z), _pd(Q), _pd(mp), _pd(mu_), _pd(pp), _pd(pu), _pd(w), commit,
                   _pd(o["z_pred"]), _pd(o["S"]), _pd(o["innov"]), _pd(o["maha"]), _pd(o["loglik"]), _pu32(o["status"]),
                   _pd(o["mu_out"]), _pd(o["cov_out"]))
        return o

    # ---- fused cycle
    def cycle(self, dt: float, meas_model: int, z, Q):
        z = _f64(z, (self.capacity, 3)); Q = _f64(Q, (self.capacity, 3, 3))
        self._call("ukfb_cycle", dt, meas_model, _pd(z), _pd(Q))

    def cycle_uniform_q(self, dt: float, meas_model: int, z, Q9):
        """fused cycle with ONE 3x3 measurement covariance for the whole batch (host arrays)"""
        z = _f64(z, (self.capacity, 3)); Q9 = _f64(Q9, (9,))
        self._call("ukfb_cycle_uniform_q", dt, meas_model, _pd(z), _pd(Q9))

    def cycle_uniform_q_dev(self, dt: float, meas_model: int, z_dev, Q9_dev):
        self._call("ukfb_cycle_uniform_q_dev", dt, meas_model, _dev(z_dev), _dev(Q9_dev))

    def update_uniform_q(self, meas_model: int, z, Q9, active=None):
        z = _f64(z, (self.capacity, 3)); Q9 = _f64(Q9, (9,))
        a = _u8(active, self.capacity)
        self._call("ukfb_update_uniform_q", meas_model, _pd(z), _pd(Q9), _pu8(a))

    def cycle_dev(self, dt: float, meas_model_uniform: int, z_dev, Q_dev, meas_model_dev=None):
        self._call("ukfb_cycle_dev", dt, meas_model_uniform, _dev_i32(meas_model_dev), _dev(z_dev), _dev(Q_dev))

    def cycle_multi_dev(self, cycles: int, dt: float, meas_model: int, z_dev, Q_dev, slots: int, first_slot: int = 0,
                        in_a_dev=None, in_b_dev=None):
        """`cycles` fused cycles in one launch, the filters stay in LDS in between; cycle c reads slot (first_slot + c) % slots
        of the device rings z_dev [slots][capacity][3], Q_dev [slots][capacity][9] and, if given, in_a_dev / in_b_dev
        [slots][capacity][3] (Pose: acceleration; Orient: acceleration, rotation rate) in place of the latched inputs."""
        self._call("ukfb_cycle_multi_dev", cycles, dt, meas_model, slots, first_slot, _dev(in_a_dev), _dev(in_b_dev), _dev(z_dev),
                   _dev(Q_dev))

    def cycle_multi_mixed_dev(self, cycles: int, dt: float, meas_model_dev, z_dev, Q_dev, slots: int, first_slot: int = 0,
                              in_a_dev=None, in_b_dev=None):
        """cycle_multi_dev with per-filter model ids per cycle: meas_model_dev int32 [slots][capacity], negative = none."""
        self._call("ukfb_cycle_multi_mixed_dev", cycles, dt, slots, first_slot, _dev(in_a_dev), _dev(in_b_dev),
                   _dev_i32(meas_model_dev), _dev(z_dev), _dev(Q_dev))

    def cycle_schedule_dev(self, dt, meas_model, z_dev, Q_dev, slots: int, first_slot: int = 0, in_a_dev=None, in_b_dev=None):
        """Scheduled multi-cycle launch: cycle c predicts by dt[c] and updates with model meas_model[c] (negative: prediction
        only); inputs from the device rings as in cycle_multi_dev."""
        d, m = _f64(dt, -1), _i32(meas_model)
        if d.size != m.size:
            raise ValueError("dt and meas_model need one entry per cycle")
        self._call("ukfb_cycle_schedule_dev", d.size, _pd(d), _pi32(m), slots, first_slot, _dev(in_a_dev), _dev(in_b_dev),
                   _dev(z_dev), _dev(Q_dev))

    def cycle_multi(self, dt: float, meas_model: int, z, Q, in_a=None, in_b=None):
        """Host arrays, one input set per cycle: z [cycles, capacity, 3], Q [cycles, capacity, 3, 3], in_a / in_b
        [cycles, capacity, 3] or None (the latched inputs); all cycles in one launch."""
        z = np.ascontiguousarray(z, dtype=np.float64)
        cycles = z.shape[0]
        z = _f64(z, (cycles, self.capacity, 3)); Q = _f64(Q, (cycles, self.capacity, 3, 3))
        a, b = _f64(in_a, (cycles, self.capacity, 3)), _f64(in_b, (cycles, self.capacity, 3))
        self._call("ukfb_cycle_multi", cycles, dt, meas_model, _pd(a), _pd(b), _pd(z), _pd(Q))

    def cycle_timestamps(self, ts_us, meas_model, z, Q):
        """Fused predictionStepFromSampleTime(ts[i]) + integrateMeasurement(model[i]); ts < 0: no sample."""
        t, m = _i64(ts_us, self.capacity), _i32(meas_model, self.capacity)
        z = _f64(z, (self.capacity, 3)); Q = _f64(Q, (self.capacity, 3, 3))
        self._call("ukfb_cycle_timestamps", _pi64(t), _pi32(m), _pd(z), _pd(Q))

    def process_events(self, filter_index, ts_us, meas_model, z, Q):
        """Time-ordered asynchronous measurement stream (any arrival order).  Returns (status_or, rounds)."""
        return _process_events(self, "ukfb_process_events", filter_index, ts_us, meas_model, z, Q)

    def process_events_dev(self, n_events: int, filter_dev, ts_us_dev, meas_model_dev, z_dev, Q_dev):
        """The same stream already resident in HBM (int64, int64, int32, z / Q in the engine's precision)."""
        st, rounds = C.c_uint32(0), C.c_int64(0)
        self._call("ukfb_process_events_dev", int(n_events), _dev_i64(filter_dev), _dev_i64(ts_us_dev), _dev_i32(meas_model_dev),
                   _dev(z_dev), _dev(Q_dev), C.byref(st), C.byref(rounds))
        return int(st.value), int(rounds.value)

    # ---- measurement of the engine
    def last_launch_info(self):
        name = C.create_string_buffer(256)
        lds, fpw, grid = C.c_int(0), C.c_int(0), C.c_int64(0)
        self._call("ukfb_last_launch_info", name, 256, C.byref(lds), C.byref(fpw), C.byref(grid))
        return {"kernel": name.value.decode(), "lds_bytes": lds.value, "filters_per_workgroup": fpw.value,
                "grid": grid.value}

    def last_model_groups(self):
        """int32 list of the most recent launch that grouped its filters by update class (-1 = padding); see ukf_batch.h"""
        items = C.c_int64(0)
        cap = int(self.capacity) + 16
        out = np.empty(cap, dtype=np.int32)
        self._call("ukfb_last_model_groups", _pi32(out), cap, C.byref(items))
        return out[:int(items.value)].copy()

    def timer_begin(self):
        self._call("ukfb_timer_begin")

    def timer_end(self) -> float:
        ms = C.c_float(0)
        self._call("ukfb_timer_end", C.byref(ms))
        return float(ms.value)


class BatchPoseUKF(BatchUKF):
    """Batched sibling of pose_estimation::PoseUKF (pose_with_velocity/PoseUKF.hpp:20-96)."""

    def __init__(self, capacity: int, precision: int = F64, device: int = 0, **kw):
        super().__init__(MODEL_POSE, precision, capacity, device, **kw)
        self.set_process_noise(_POSE_DEFAULT_NOISE)


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
        _latch_orient_inputs(self, mu, first)


class _ShardView(BatchUKF):
    """A shard's engine seen through the per-engine binding (the group owns the handle: close() is a no-op)."""

    def __init__(self, lib, handle, model, precision, capacity, device):   # noqa: D401 (no ukfb_create here)
        self._lib, self._h = lib, handle
        self.model, self.precision, self.capacity, self.device = model, precision, int(capacity), device
        self.S, self.D, self.PK, self.dtype = _dims(model, precision)
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
        _invoke(self._lib, "ukfb_group_create", C.byref(self._g), model, precision, total, devs, len(devices))
        self.model, self.precision, self.total = model, precision, int(total)
        self.S, self.D, self.PK, self.dtype = _dims(model, precision)
        self.n = int(self._lib.ukfb_group_size(self._g))
        self.shards = []
        for r in range(self.n):
            h, dev, first, count = C.c_void_p(), C.c_int(0), C.c_int64(0), C.c_int64(0)
            self._call("ukfb_group_shard", r, C.byref(h), C.byref(dev), C.byref(first), C.byref(count))
            self.shards.append({"engine": _ShardView(self._lib, h, model, precision, count.value, dev.value),
                                "device": dev.value, "first": first.value, "count": count.value})
        if model == MODEL_POSE:   # as BatchPoseUKF
            self.set_process_noise(_POSE_DEFAULT_NOISE)

    def _call(self, name: str, *args):
        """The entry point `name` on this group's handle."""
        _invoke(self._lib, name, self._g, *args)

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
        return (C.c_void_p * self.n)(*[_dev(x) for x in xs])

    def configure(self, **kw):
        c = self.shards[0]["engine"].config()
        for k, v in kw.items():
            setattr(c, k, v)
        self._call("ukfb_group_set_config", C.byref(c))

    def initialize(self, mu, cov, first: int = 0):
        mu = _f64(mu, (-1, self.S)); cov = _f64(cov, (-1, self.D, self.D))
        self._call("ukfb_group_initialize", first, mu.shape[0], _pd(mu), _pd(cov))
        if self.model == MODEL_ORIENT:   # as BatchOrientationUKF
            _latch_orient_inputs(self, mu, first)

    def state(self, first: int = 0, count: Optional[int] = None):
        count = self.total - first if count is None else count
        mu = np.empty((count, self.S)); cov = np.empty((count, self.D, self.D)); init = np.empty(count, dtype=np.uint8)
        self._call("ukfb_group_get_state", first, count, _pd(mu), _pd(cov), _pu8(init))
        return mu, cov, init.astype(bool)

    def status(self, first: int = 0, count: Optional[int] = None):
        count = self.total - first if count is None else count
        st = np.empty(count, dtype=np.uint32)
        self._call("ukfb_group_get_status", first, count, _pu32(st))
        return st

    def status_summary(self) -> int:
        v = C.c_uint32(0)
        self._call("ukfb_group_get_status_summary", C.byref(v))
        return int(v.value)

    def set_process_noise(self, R):
        self._call("ukfb_group_set_process_noise", _pd(_f64(R, (self.D, self.D))))

    def set_acceleration(self, acc_mu=None, acc_cov=None, first: int = 0):
        am, ac = _f64(acc_mu, (-1, 3)), _f64(acc_cov, (3, 3))
        self._call("ukfb_group_pose_set_acceleration", first, am.shape[0] if am is not None else 0, _pd(am), _pd(ac))

    def set_orient_params(self, gyro_bias_tau: float, acc_bias_tau: float, earth_rotation):
        self._call("ukfb_group_orient_set_params", gyro_bias_tau, acc_bias_tau, _pd(_f64(earth_rotation, (3,))))

    def set_orient_inputs(self, gyro=None, acc=None, first: int = 0):
        g, a = _f64(gyro, (-1, 3)), _f64(acc, (-1, 3))
        n = g.shape[0] if g is not None else (a.shape[0] if a is not None else 0)
        self._call("ukfb_group_orient_set_inputs", first, n, _pd(g), _pd(a))

    def predict(self, dt: float):
        self._call("ukfb_group_predict", dt)

    def update(self, meas_model: int, z, Q):
        z = _f64(z, (self.total, 3)); Q = _f64(Q, (self.total, 3, 3))
        self._call("ukfb_group_update", meas_model, _pd(z), _pd(Q))

    def cycle(self, dt: float, meas_model: int, z, Q):
        z = _f64(z, (self.total, 3)); Q = _f64(Q, (self.total, 3, 3))
        self._call("ukfb_group_cycle", dt, meas_model, _pd(z), _pd(Q))

    def bind_acceleration_dev(self, acc_devs):
        self._call("ukfb_group_pose_bind_acceleration_dev", self._ptrs(acc_devs))

    def bind_orient_inputs_dev(self, gyro_devs, acc_devs):
        self._call("ukfb_group_orient_bind_inputs_dev", self._ptrs(gyro_devs), self._ptrs(acc_devs))

    def cycle_dev(self, dt: float, meas_model: int, z_devs, Q_devs):
        self._call("ukfb_group_cycle_dev", dt, meas_model, self._ptrs(z_devs), self._ptrs(Q_devs))

    def cycle_multi_dev(self, cycles: int, dt: float, meas_model: int, z_devs, Q_devs, slots: int, first_slot: int = 0,
                        in_a_devs=None, in_b_devs=None):
        self._call("ukfb_group_cycle_multi_dev", cycles, dt, meas_model, slots, first_slot, self._ptrs(in_a_devs),
                   self._ptrs(in_b_devs), self._ptrs(z_devs), self._ptrs(Q_devs))

    def cycle_mixed_dev(self, dt: float, meas_model_devs, z_devs, Q_devs):
        """per-filter model ids resident on the devices (int32, one array per shard)"""
        self._call("ukfb_group_cycle_mixed_dev", dt, self._ptrs(meas_model_devs), self._ptrs(z_devs), self._ptrs(Q_devs))

    def cycle_timestamps(self, ts_us, meas_model, z, Q):
        t, m = _i64(ts_us, self.total), _i32(meas_model, self.total)
        z = _f64(z, (self.total, 3)); Q = _f64(Q, (self.total, 3, 3))
        self._call("ukfb_group_cycle_timestamps", _pi64(t), _pi32(m), _pd(z), _pd(Q))

    def process_events(self, filter_index, ts_us, meas_model, z, Q):
        """Time-ordered asynchronous stream over the sharded batch (filter indices in batch numbering, any arrival order).
        Returns (status_or, rounds of the shard that needed most)."""
        return _process_events(self, "ukfb_group_process_events", filter_index, ts_us, meas_model, z, Q)

    def sync(self):
        self._call("ukfb_group_sync")

    def timer_begin(self):
        self._call("ukfb_group_timer_begin")

    def timer_end(self):
        """(slowest shard's ms, [ms per shard])"""
        mx = C.c_float(0)
        per = (C.c_float * self.n)()
        self._call("ukfb_group_timer_end", C.byref(mx), per)
        return float(mx.value), [float(x) for x in per]

    def gather_means(self, out_devs):
        """RCCL all-gather of the means: out_devs[r] = device buffer [total][S] (engine precision) on shard r's device."""
        self._call("ukfb_group_gather_means", self._ptrs(out_devs))

    def last_gather_exchange(self) -> str:
        """which exchange the last gather_means used: "rccl" (one shard per device) or "copies" (shards sharing a device)"""
        return {0: "none", 1: "rccl", 2: "copies"}.get(int(self._lib.ukfb_group_last_gather_exchange(self._g)), "?")


