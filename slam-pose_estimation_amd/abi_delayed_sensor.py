"""The C ABI of include/ukf_batch_delayed_sensor.h (late sensor-frame samples) as ctypes sees it: the structure and SIGNATURES,
the result and argument types of its entry points.  An extension of abi.py in a module of its own, as the header is an
extension of ukf_batch.h: abi.py states ukf_batch.h and nothing else.  The model ids are abi.py's SENSOR_*, the outputs its
DelayedOut.  tests/test_delayed_sensor_host.py holds this file to the header type by type, with abi.py's rules."""
from __future__ import annotations

import ctypes as C

from .abi import DelayedOut, _h, _i, _P, _pd, _pi32, _pu32


class DelayedSensorIn(C.Structure):
    """ukfb_delayed_sensor_in: the delayed update's window (dt a HOST array) and lags, then the sensor-frame sample: model, z [3],
    Q [9], mount, point (host values by value, or device arrays per filter) and the rotation rate at the time of the sample;
    device pointers in engine precision"""
    _fields_ = [("steps", C.c_int), ("dt", C.POINTER(C.c_double)), ("slots", C.c_int), ("first_slot", C.c_int),
                ("mu_hist_dev", C.c_void_p), ("cov_hist_dev", C.c_void_p), ("in_a_dev", C.c_void_p), ("in_b_dev", C.c_void_p),
                ("lag_uniform", C.c_int), ("lag_dev", C.c_void_p), ("model_uniform", C.c_int), ("model_dev", C.c_void_p),
                ("z_dev", C.c_void_p), ("Q_dev", C.c_void_p), ("q_is_uniform", C.c_int),
                ("mount_dev", C.c_void_p), ("mount_uniform", C.c_double * 7), ("point_dev", C.c_void_p),
                ("point_uniform", C.c_double * 3), ("rate_dev", C.c_void_p)]


# entry point -> (restype, argtypes), in the header's order
SIGNATURES = {
    "ukfb_update_delayed_sensor_dev": (_i, (_h, _P(DelayedSensorIn), _i, _P(DelayedOut))),
    "ukfb_update_delayed_sensor": (_i, (_h, _i, _pd, _pd, _pd, _pd, _pd, _i, _pi32, _i, _pi32, _pd, _pd, _pd, _pd, _pd, _pd, _pd, _i,
                                        _pd, _pd, _pd, _pd, _pd, _pu32, _pd, _pd)),
}

# every symbol include/ukf_batch_delayed_sensor.h declares
EXPORTS = list(SIGNATURES)


def declare(lib):
    """Set restype and argtypes on every entry point of a loaded CDLL; a missing symbol raises AttributeError."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
