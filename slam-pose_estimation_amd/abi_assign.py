"""The C ABI of include/ukf_batch_assign.h (the assignment across the filters of a scene) as ctypes sees it: the two structures,
the constants and SIGNATURES, the result and argument types of its entry points.  An extension of abi.py in a module of its own,
as the header is an extension of ukf_batch.h: abi.py states ukf_batch.h and nothing else.  tests/test_assign_host.py holds this
file to the header type by type, with abi.py's rules."""
from __future__ import annotations

import ctypes as C

from .abi import _d, _h, _i, _P, _pd, _pi32, _pu32

# most tracks of a scene (UKFB_ASSIGN_MAX_TRACKS), the largest |cost| and |miss| that take part (UKFB_ASSIGN_COST_MAX), and the
# values of scene_status
ASSIGN_MAX_TRACKS = 32
ASSIGN_COST_MAX = 1e100
ASSIGN_OK, ASSIGN_BAD_SCENE = 0, 1


class AssignIn(C.Structure):
    """ukfb_assign_in: cost [candidates, capacity] and miss [capacity] device pointers in engine precision, scene_start int32
    [scenes + 1] (NULL: uniform scenes of tracks_per_scene slots); gate and miss_uniform host doubles"""
    _fields_ = [("cost_dev", C.c_void_p), ("candidates", C.c_int), ("scenes", C.c_int), ("scene_start_dev", C.c_void_p),
                ("tracks_per_scene", C.c_int), ("gate", C.c_double), ("miss_dev", C.c_void_p), ("miss_uniform", C.c_double)]


class AssignOut(C.Structure):
    """ukfb_assign_out: device pointers (assign, owner int32; objective double; scene_status uint32), any may be NULL, not all"""
    _fields_ = [("assign", C.c_void_p), ("owner", C.c_void_p), ("objective", C.c_void_p), ("scene_status", C.c_void_p)]


# entry point -> (restype, argtypes), in the header's order
SIGNATURES = {
    "ukfb_assign_scenes_dev": (_i, (_h, _P(AssignIn), _P(AssignOut))),
    "ukfb_assign_scenes": (_i, (_h, _i, _pd, _i, _pi32, _i, _d, _pd, _d, _pi32, _pi32, _pd, _pu32)),
}

# every symbol include/ukf_batch_assign.h declares
EXPORTS = list(SIGNATURES)


def declare(lib):
    """Set restype and argtypes on every entry point of a loaded CDLL; a missing symbol raises AttributeError."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
