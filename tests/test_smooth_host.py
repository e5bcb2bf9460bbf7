"""The smoother's entry points without a GPU: the symbols of include/ukf_batch.h are exported and bound, the host decisions of
ukf_host.hpp (check_smooth_args, check_history_args, SmoothPlan, smooth_geometry) hold under ASan / UBSan
(tests/cpp/smooth_host.cpp, compiled here), and a NULL engine is refused before anything touches a device."""
import ctypes as C

from host_support import header_text, run_sanitized

NAMES = ("ukfb_history_push_dev", "ukfb_smooth_dev", "ukfb_smooth")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("history_push_dev", "smooth_dev", "smooth"):
        assert callable(getattr(spe.BatchUKF, method))


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    dt = (C.c_double * 1)(0.01); buf = (C.c_double * 512)()
    assert lib.ukfb_history_push_dev(None, C.c_int(2), C.c_int(0), buf, buf) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_smooth_dev(None, C.c_int(2), dt, C.c_int(2), C.c_int(0), buf, buf, None, None, buf, None, None) == 1
    assert lib.ukfb_smooth(None, C.c_int(2), dt, buf, buf, None, None, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("smooth_host.cpp", tmp_path)
