"""The sensor-frame measurements without a GPU: the symbols of include/ukf_batch.h are exported and bound, the host decisions
of ukf_host.hpp (check_sensor_args, the model ids per engine, sensor_meas_dim, which inputs a model reads, sensor_geometry)
hold under ASan / UBSan (tests/cpp/sensor_meas_host.cpp, compiled here as a stand-alone program), and a NULL engine is refused
before anything touches a device."""
import ctypes as C
import os

from host_support import header_text, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_update_sensor_dev", "ukfb_update_sensor")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("update_sensor_dev", "update_sensor"):
        assert callable(getattr(spe.BatchUKF, method))
    assert "ukfb_sensor_in" in header and "ukfb_sensor_out" in header
    assert [f[0] for f in spe.SensorIn._fields_] == ["model_dev", "z_dev", "Q_dev", "q_is_uniform", "mount_dev", "mount_uniform",
                                                     "point_dev", "point_uniform"]
    assert [f[0] for f in spe.SensorOut._fields_] == ["z_pred", "S", "innov", "maha", "loglik", "status"]
    assert C.sizeof(spe.SensorIn) == 8 * 3 + 8 + 8 + 7 * 8 + 8 + 3 * 8 and C.sizeof(spe.SensorOut) == 6 * 8
    names = ("POSE_POSITION", "POSE_RANGE", "POSE_POINT", "POSE_VELOCITY", "POSE_NAV_VELOCITY", "ORIENT_VELOCITY",
             "ORIENT_NAV_VECTOR", "ORIENT_SPECIFIC_FORCE")
    for value, name in enumerate(names):
        assert getattr(spe, "SENSOR_" + name) == value and f"UKFB_SENSOR_{name} = {value}" in header
    assert spe.SENSOR_NONE == -1
    batch = open(os.path.join(ROOT, "include", "pose_estimation", "Batch.hpp")).read()
    assert "integrateSensorMeasurement(" in batch and "ukfb_update_sensor(" in batch


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    buf = (C.c_double * 64)()
    addr = C.addressof(buf)
    sin = spe.SensorIn(None, addr, addr, 0, None, (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1), None, (C.c_double * 3)())
    out = spe.SensorOut(None, None, None, None, None, None)
    assert lib.ukfb_update_sensor_dev(None, C.c_int(0), C.byref(sin), C.c_int(1), C.byref(out)) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_update_sensor(None, C.c_int(0), None, buf, buf, None, None, None, None, C.c_int(1), None, None, None, None,
                                  None, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("sensor_meas_host.cpp", tmp_path)
