"""The C ABI of include/ukf_batch_jpda.h (the joint association marginals of a scene and the update with given weights) as
ctypes sees it: the three structures, the constants and SIGNATURES, the result and argument types of its entry points.  An
extension of abi.py in a module of its own, as the header is an extension of ukf_batch.h: abi.py states ukf_batch.h and nothing
else.  tests/test_jpda_host.py holds this file to the header type by type, with abi.py's rules."""
from __future__ import annotations

import ctypes as C

from .abi import AssociateIn, _d, _h, _i, _P, _pd, _pi32, _pu32
from .abi_pda import PdaRule

# most tracks of a scene (UKFB_JPDA_MAX_TRACKS), the cap of ln psi (UKFB_JPDA_LOG_RATIO_MAX), and the values of scene_status
JPDA_MAX_TRACKS = 6
JPDA_LOG_RATIO_MAX = 100.0
JPDA_OK, JPDA_BAD_SCENE, JPDA_TOO_LARGE = 0, 1, 2


class JpdaIn(C.Structure):
    """ukfb_jpda_in: loglik and maha [candidates, capacity] device pointers in engine precision (maha may be NULL without a
    gate), scene_start int32 [scenes + 1] (NULL: uniform scenes of tracks_per_scene slots), gate a host double, the sensor
    model of the tracks (model_dev int32 [capacity], or model_uniform)"""
    _fields_ = [("loglik_dev", C.c_void_p), ("maha_dev", C.c_void_p), ("candidates", C.c_int), ("scenes", C.c_int),
                ("scene_start_dev", C.c_void_p), ("tracks_per_scene", C.c_int), ("gate", C.c_double), ("model_uniform", C.c_int),
                ("model_dev", C.c_void_p)]


class JpdaOut(C.Structure):
    """ukfb_jpda_out: device pointers (beta, beta0 engine precision; free, log_z double; scene_status uint32), any may be NULL,
    not all"""
    _fields_ = [("beta", C.c_void_p), ("beta0", C.c_void_p), ("free", C.c_void_p), ("log_z", C.c_void_p), ("scene_status", C.c_void_p)]


class WeightedOut(C.Structure):
    """ukfb_weighted_out: device pointers in engine precision (n_used int32, status uint32), any may be NULL"""
    _fields_ = [("z_pred", C.c_void_p), ("S", C.c_void_p), ("innov", C.c_void_p), ("maha", C.c_void_p), ("loglik", C.c_void_p),
                ("weight_used", C.c_void_p), ("beta0", C.c_void_p), ("innov_comb", C.c_void_p), ("n_used", C.c_void_p),
                ("status", C.c_void_p)]


# entry point -> (restype, argtypes), in the header's order
SIGNATURES = {
    "ukfb_jpda_scenes_dev": (_i, (_h, _P(JpdaIn), _P(PdaRule), _P(JpdaOut))),
    "ukfb_jpda_scenes": (_i, (_h, _i, _pd, _pd, _i, _pi32, _i, _d, _i, _pi32, _P(PdaRule), _pd, _pd, _pd, _pd, _pu32)),
    "ukfb_update_weighted_dev": (_i, (_h, _i, _P(AssociateIn), _h, _i, _P(WeightedOut))),
    "ukfb_update_weighted": (_i, (_h, _i, _pi32, _i, _pd, _pd, _pd, _pd, _pd, _pd, _pd, _i, _pd, _pd, _pd, _pd, _pd, _pd, _pd, _pd,
                                  _pi32, _pu32)),
}

# every symbol include/ukf_batch_jpda.h declares
EXPORTS = list(SIGNATURES)


def declare(lib):
    """Set restype and argtypes on every entry point of a loaded CDLL; a missing symbol raises AttributeError."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
