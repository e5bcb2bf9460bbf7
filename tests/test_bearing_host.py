"""The bearing measurements without a GPU: the symbols of include/ukf_batch.h are exported and bound, the enum values, the
methods of Batch.hpp, the host decisions of ukf_host.hpp (bearing_model_ok, bearing_input_used, check_bearing_args, the LDS
accounting and launch geometry of the kernel) hold under ASan / UBSan (tests/cpp/bearing_host.cpp, compiled here as a
stand-alone program), and a NULL engine is refused before anything touches a device."""
import ctypes as C
import os
import re

from host_support import header_text, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_update_bearing_dev", "ukfb_update_bearing")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("update_bearing_dev", "update_bearing"):
        assert callable(getattr(spe.BatchUKF, method))
    for name, value in (("NONE", -1), ("POSE_POINT", 0), ("POSE_NAV_DIRECTION", 1), ("ORIENT_NAV_DIRECTION", 2)):
        assert re.search(r"UKFB_BEARING_%s = %d\b" % (name, value), header), name
        assert getattr(spe.engine, "BEARING_" + name) == value
    # the section stands after the sensor-frame measurements, whose structs it reuses
    assert header.index("sensor-frame measurements: lever arms") < header.index("bearing measurements: directions on the sphere")
    assert header.index("enum ukfb_bearing_model") < header.index("user-defined measurement models: sigma-point export")
    batch = open(os.path.join(ROOT, "include", "pose_estimation", "Batch.hpp")).read()
    assert "integrateBearingMeasurementDev(int model_uniform, const ukfb_sensor_in& in, bool commit = true" in batch
    assert "integrateBearingMeasurement(" in batch and "ukfb_update_bearing(" in batch and "ukfb_update_bearing_dev(" in batch
    tool = open(os.path.join(ROOT, "tools", "check_resources.py")).read()
    assert tool.count("ukf_bearing_kernel") >= 2  # gated, and held to its two wavefronts per SIMD


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    buf = (C.c_double * 64)()
    addr = C.addressof(buf)
    sin = spe.SensorIn(None, addr, addr, 0, None, (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1), None, (C.c_double * 3)(1, 0, 0))
    out = spe.SensorOut(None, None, None, addr, None, None)
    for commit in (0, 1):
        assert lib.ukfb_update_bearing_dev(None, C.c_int(0), C.byref(sin), C.c_int(commit), C.byref(out)) == 1   # UKFB_ERR_INVALID_ARG
    pd = C.POINTER(C.c_double)
    z = C.cast(buf, pd)
    assert lib.ukfb_update_bearing(None, C.c_int(0), None, z, z, None, None, None, None, C.c_int(1), None, None, None, z, None, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("bearing_host.cpp", tmp_path)
