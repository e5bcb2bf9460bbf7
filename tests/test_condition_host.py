"""The covariance conditioning without a GPU: the symbols of include/ukf_batch.h are exported and bound, the host decisions of
ukf_host.hpp (check_condition_args, check_condition_floor, the schedule's counts, the LDS accounting and launch geometry of the
kernel) hold under ASan / UBSan (tests/cpp/condition_host.cpp, compiled here as a stand-alone program), and a NULL engine is
refused before anything touches a device."""
import ctypes as C
import os

from host_support import header_text, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_condition_dev", "ukfb_condition")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("condition_dev", "condition"):
        assert callable(getattr(spe.BatchUKF, method))
    assert "ukfb_condition_in" in header and "ukfb_condition_out" in header and "UKFB_ST_REPAIRED = 1u << 11" in header
    assert spe.engine.ST_REPAIRED == 1 << 11
    assert [f[0] for f in spe.ConditionIn._fields_] == ["var_floor_dev", "eig_floor", "select_dev", "renormalize_quaternion"]
    assert [f[0] for f in spe.ConditionOut._fields_] == ["eig_min", "eig_max", "mu", "cov_packed", "status"]
    assert C.sizeof(spe.ConditionIn) == 8 + 8 + 8 + 8 and C.sizeof(spe.ConditionOut) == 5 * 8
    assert spe.ConditionIn.eig_floor.offset == 8 and spe.ConditionIn.select_dev.offset == 16
    assert spe.ConditionIn.renormalize_quaternion.offset == 24
    batch = open(os.path.join(ROOT, "include", "pose_estimation", "Batch.hpp")).read()
    assert "condition(" in batch and "conditionDev(" in batch
    assert "ukfb_condition(" in batch and "ukfb_condition_dev(" in batch


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    buf = (C.c_double * 64)()
    addr = C.addressof(buf)
    cin = spe.ConditionIn(addr, 1e-4, None, 0)
    out = spe.ConditionOut(None, None, None, None, None)
    assert lib.ukfb_condition_dev(None, C.byref(cin), C.c_int(1), C.byref(out)) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_condition_dev(None, C.byref(cin), C.c_int(0), C.byref(out)) == 1
    assert lib.ukfb_condition(None, buf, C.c_double(1e-4), None, C.c_int(0), C.c_int(1), None, None, None, None, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("condition_host.cpp", tmp_path)
