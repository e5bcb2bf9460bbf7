"""The C ABI of include/ukf_batch_pda.h (the probabilistic data association update) as ctypes sees it: the two structures and
SIGNATURES, the result and argument types of its entry points.  An extension of abi.py in a module of its own, as the header is
an extension of ukf_batch.h: abi.py states ukf_batch.h and nothing else.  tests/test_pda_host.py holds this file to the header
type by type, with abi.py's rules."""
from __future__ import annotations

import ctypes as C

from .abi import AssociateIn, _h, _i, _P, _pd, _pi32, _pu32


class PdaRule(C.Structure):
    """ukfb_pda_rule: host values -- the detection probability P_D, the gate probabilities P_G for m = 1 and m = 3, and the
    clutter densities lambda (per unit volume of the measurement space) for m = 1 and m = 3"""
    _fields_ = [("p_detect", C.c_double), ("p_gate_m1", C.c_double), ("p_gate_m3", C.c_double), ("clutter_m1", C.c_double),
                ("clutter_m3", C.c_double)]


class PdaOut(C.Structure):
    """ukfb_pda_out: device pointers in engine precision (best, n_gated int32, status uint32), any may be NULL"""
    _fields_ = [("z_pred", C.c_void_p), ("S", C.c_void_p), ("innov", C.c_void_p), ("maha", C.c_void_p), ("loglik", C.c_void_p),
                ("beta", C.c_void_p), ("beta0", C.c_void_p), ("innov_comb", C.c_void_p), ("best", C.c_void_p), ("n_gated", C.c_void_p),
                ("status", C.c_void_p)]


# entry point -> (restype, argtypes), in the header's order
SIGNATURES = {
    "ukfb_update_pda_dev": (_i, (_h, _i, _P(AssociateIn), _P(PdaRule), _i, _P(PdaOut))),
    "ukfb_update_pda": (_i, (_h, _i, _pi32, _i, _pd, _pd, _pd, _pd, _pd, _pd, _P(PdaRule), _i, _pd, _pd, _pd, _pd, _pd, _pd, _pd, _pd,
                             _pi32, _pi32, _pu32)),
}

# every symbol include/ukf_batch_pda.h declares
EXPORTS = list(SIGNATURES)


def declare(lib):
    """Set restype and argtypes on every entry point of a loaded CDLL; a missing symbol raises AttributeError."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
