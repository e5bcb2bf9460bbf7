"""The C ABI of include/ukf_batch_robust.h (the robust sensor-frame update) as ctypes sees it: the constants, the two
structures and SIGNATURES, the result and argument types of its entry points.  An extension of abi.py in a module of its own, as
the header is an extension of ukf_batch.h: abi.py states ukf_batch.h and nothing else.  tests/test_robust_host.py holds this
file to the header type by type, with abi.py's rules."""
from __future__ import annotations

import ctypes as C

from .abi import SensorIn, _h, _i, _P, _pd, _pi32, _pu32

# modes of ukfb_robust_rule
ROBUST_MATCH, ROBUST_HUBER = 0, 1


class RobustRule(C.Structure):
    """ukfb_robust_rule: host values -- the mode, the thresholds c^2 for m = 1 and m = 3, the clamp of lambda, and for MATCH the
    relative tolerance on d^2(lambda) - c^2 and the cap on Newton steps"""
    _fields_ = [("mode", C.c_int), ("chi2_m1", C.c_double), ("chi2_m3", C.c_double), ("scale_max", C.c_double), ("tol", C.c_double),
                ("max_iter", C.c_int)]


class RobustOut(C.Structure):
    """ukfb_robust_out: device pointers in engine precision (iterations int32, status uint32), any may be NULL"""
    _fields_ = [("z_pred", C.c_void_p), ("S", C.c_void_p), ("innov", C.c_void_p), ("maha0", C.c_void_p), ("maha", C.c_void_p),
                ("loglik", C.c_void_p), ("scale", C.c_void_p), ("iterations", C.c_void_p), ("status", C.c_void_p)]


# entry point -> (restype, argtypes), in the header's order
SIGNATURES = {
    "ukfb_update_robust_dev": (_i, (_h, _i, _P(SensorIn), _P(RobustRule), _i, _P(RobustOut))),
    "ukfb_update_robust": (_i, (_h, _i, _pi32, _pd, _pd, _pd, _pd, _pd, _pd, _P(RobustRule), _i, _pd, _pd, _pd, _pd, _pd, _pd, _pd, _pi32, _pu32)),
}

# every symbol include/ukf_batch_robust.h declares
EXPORTS = list(SIGNATURES)


def declare(lib):
    """Set restype and argtypes on every entry point of a loaded CDLL; a missing symbol raises AttributeError."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
