"""The C ABI of include/ukf_batch_relative.h (relative measurements) as ctypes sees it: the constants, the two structures and
SIGNATURES, the result and argument types of its entry points.  An extension of abi.py in a module of its own, as the header
is an extension of ukf_batch.h: abi.py states ukf_batch.h and nothing else.  tests/test_relative_host.py holds this file to
the header type by type, with abi.py's rules."""
from __future__ import annotations

import ctypes as C

from .abi import _h, _i, _P, _pd, _pi32, _pu32

# models of ukfb_update_relative_dev (Pose engines)
RELATIVE_NONE = -1
RELATIVE_POSE, RELATIVE_POSITION, RELATIVE_ROTATION = 0, 1, 2


class RelativeIn(C.Structure):
    """ukfb_relative_in: the delayed update's window (dt a HOST array) and lags, the relative model and the increment z [7], Q [36];
    device pointers in engine precision"""
    _fields_ = [("steps", C.c_int), ("dt", C.POINTER(C.c_double)), ("slots", C.c_int), ("first_slot", C.c_int),
                ("mu_hist_dev", C.c_void_p), ("cov_hist_dev", C.c_void_p), ("in_a_dev", C.c_void_p), ("in_b_dev", C.c_void_p),
                ("lag_uniform", C.c_int), ("lag_dev", C.c_void_p), ("model_uniform", C.c_int), ("model_dev", C.c_void_p),
                ("z_dev", C.c_void_p), ("Q_dev", C.c_void_p), ("q_is_uniform", C.c_int)]


class RelativeOut(C.Structure):
    """ukfb_relative_out: device pointers in engine precision (status uint32), any may be NULL"""
    _fields_ = [("z_pred", C.c_void_p), ("S", C.c_void_p), ("innov", C.c_void_p), ("maha", C.c_void_p), ("loglik", C.c_void_p),
                ("status", C.c_void_p), ("mu_out", C.c_void_p), ("cov_out", C.c_void_p)]


# entry point -> (restype, argtypes), in the header's order
SIGNATURES = {
    "ukfb_update_relative_dev": (_i, (_h, _P(RelativeIn), _i, _P(RelativeOut))),
    "ukfb_update_relative": (_i, (_h, _i, _pd, _pd, _pd, _pd, _pd, _i, _pi32, _i, _pi32, _pd, _pd, _i, _pd, _pd, _pd, _pd, _pd, _pu32, _pd, _pd)),
}

# every symbol include/ukf_batch_relative.h declares
EXPORTS = list(SIGNATURES)


def declare(lib):
    """Set restype and argtypes on every entry point of a loaded CDLL; a missing symbol raises AttributeError."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
