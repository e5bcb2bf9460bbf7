"""The forecast's entry points without a GPU: the symbols of include/ukf_batch.h are exported and bound, the host decisions of
ukf_host.hpp (check_forecast_args, forecast_filter_scalars, forecast_geometry) hold under ASan / UBSan
(tests/cpp/forecast_host.cpp, compiled here as a stand-alone program), and a NULL engine is refused before anything touches a
device."""
import ctypes as C
import os

from host_support import header_text, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_forecast_dev", "ukfb_forecast")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("forecast_dev", "forecast"):
        assert callable(getattr(spe.BatchUKF, method))
    assert "#define UKFB_FORECAST_MAX_STEPS 32" in header
    section = header[header.index("---- forecast"):header.index("int ukfb_forecast(")]
    for text in ("(first_slot + c) % slots", "READ-ONLY", "must not alias", "UKFB_ERR_OUT_OF_RANGE", "SKIPPED_FIRST_TS",
                 "exactly as ukfb_predict makes it", "ukfb_group_shard"):
        assert text in section, text
    batch = open(os.path.join(ROOT, "include", "pose_estimation", "Batch.hpp")).read()
    assert "forecast(" in batch and "ukfb_forecast(" in batch


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    dt = (C.c_double * 1)(0.01); buf = (C.c_double * 512)()
    assert lib.ukfb_forecast_dev(None, C.c_int(1), dt, None, C.c_int(2), C.c_int(0), None, None, None, None, buf, None, None) == 1
    assert lib.ukfb_forecast(None, C.c_int(1), dt, None, None, None, None, None, buf, None, None) == 1   # UKFB_ERR_INVALID_ARG


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("forecast_host.cpp", tmp_path)
