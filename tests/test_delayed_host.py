"""The delayed-measurement update's entry points without a GPU: the symbols of include/ukf_batch.h are exported, bound and
documented, the host decisions of ukf_host.hpp (check_delayed_args, check_delayed_lag_args, delayed_geometry, the lag rule) hold
under ASan / UBSan (tests/cpp/delayed_host.cpp, compiled here as a stand-alone program), the lag rule of the C++ side is the one
of tests/delayed_reference.py, and a NULL engine is refused before anything touches a device."""
import ctypes as C
import os

import numpy as np

import delayed_reference as dr
from host_support import header_text, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_update_delayed_dev", "ukfb_update_delayed", "ukfb_delayed_lag_dev")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("update_delayed_dev", "update_delayed", "delayed_lag_dev"):
        assert callable(getattr(spe.BatchUKF, method))
    section = header[header.index("---- late samples"):header.index("int ukfb_delayed_lag_dev(")]
    for text in ("STEP n = steps - 1 IS", "never read", "UKFB_DELAYED_MAX_STEPS", "UKFB_ERR_OUT_OF_RANGE", "UKFB_ST_ERR_NEG_DT", "INACTIVE",
                 "M_c = A(delta_c,rot) G_c J(e_rot) M_(c+1)", "Y_n = Sigma_n M_s^T (Sigma^s_s)^-1 Y_s", "REFUSES the sample",
                 "The residual offset", "LIMITATION: the ring is not rewritten", "must NOT be the engine's own arrays",
                 "READ-ONLY", "ukfb_group_shard", "ties go to the OLDER step"):
        assert text in section, text
    # the bindings' structs have the header's fields, in its order
    for cls, tag in ((spe.engine.DelayedIn, "ukfb_delayed_in"), (spe.engine.DelayedOut, "ukfb_delayed_out")):
        struct = header[header.index("typedef struct " + tag):header.index("} " + tag + ";")]
        fields = [f[0] for f in cls._fields_]
        pos = [min(struct.index(s + f + e) for s in (" ", "*") for e in (";", ",") if (s + f + e) in struct) for f in fields]
        assert pos == sorted(pos), (tag, fields)
    assert C.sizeof(spe.engine.DelayedOut) == 8 * C.sizeof(C.c_void_p)
    batch = open(os.path.join(ROOT, "include", "pose_estimation", "Batch.hpp")).read()
    for call in ("ukfb_update_delayed_dev(", "ukfb_update_delayed(", "ukfb_delayed_lag_dev("):
        assert call in batch, call
    for method in ("updateDelayedDev(", "updateDelayed(", "delayedLagDev("):
        assert method in batch, method


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    din, out = spe.engine.DelayedIn(), spe.engine.DelayedOut()
    ts = (C.c_int64 * 4)(1, 2, 3, 4)
    assert lib.ukfb_update_delayed_dev(None, C.byref(din), C.c_int(1), C.byref(out)) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_delayed_lag_dev(None, C.c_int(4), ts, None, None) == 1
    assert lib.ukfb_update_delayed(None, C.c_int(2), None, None, None, None, None, C.c_int(1), None, C.c_int(0), None, None, None,
                                   C.c_int(1), None, None, None, None, None, None, None, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("delayed_host.cpp", tmp_path)


def test_the_reference_states_the_same_lag_rule():
    """tests/cpp/delayed_host.cpp pins delayed_lag_of on these stamps; tests/delayed_reference.lag_rule must give the same"""
    ts = np.array([1000, 2000, 3100, 4000, 5000], dtype=np.int64)
    t = np.array([5000, 9000, 4999, 4500, 4501, 3550, 1000, 600, 500, 499, -7000, 2550, 1500], dtype=np.int64)
    assert list(dr.lag_rule(ts, t)) == [0, 0, 0, 1, 0, 2, 4, 4, 4, 5, 5, 3, 4]
    assert list(dr.lag_rule(ts[:1], np.array([1000, 2000, 999]))) == [0, 0, 1]
