"""The user-defined process models without a GPU: the symbols of include/ukf_batch.h are exported and bound, the host decisions
of ukf_host.hpp (check_predict_sampled_args, the LDS accounting and launch geometry of the kernel) hold under ASan / UBSan
(tests/cpp/predict_sampled_host.cpp, compiled here as a stand-alone program), and a NULL engine is refused before anything
touches a device."""
import ctypes as C
import os

from host_support import header_text, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_predict_sampled_dev", "ukfb_predict_sampled")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("predict_sampled_dev", "predict_sampled"):
        assert callable(getattr(spe.BatchUKF, method))
    assert "ukfb_predict_sampled_in" in header and "ukfb_predict_sampled_out" in header
    assert [f[0] for f in spe.PredictSampledIn._fields_] == ["XX_dev", "R_dev", "r_is_uniform", "active_dev"]
    assert [f[0] for f in spe.PredictSampledOut._fields_] == ["mu", "cov_packed", "status"]
    assert C.sizeof(spe.PredictSampledIn) == 2 * 8 + 8 + 8 and C.sizeof(spe.PredictSampledOut) == 3 * 8
    assert spe.PredictSampledIn.r_is_uniform.offset == 16 and spe.PredictSampledIn.active_dev.offset == 24
    batch = open(os.path.join(ROOT, "include", "pose_estimation", "Batch.hpp")).read()
    assert "predictSampled(" in batch and "predictSampledDev(" in batch
    assert "ukfb_predict_sampled(" in batch and "ukfb_predict_sampled_dev(" in batch


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    buf = (C.c_double * 64)()
    addr = C.addressof(buf)
    pin = spe.PredictSampledIn(addr, addr, 0, None)
    out = spe.PredictSampledOut(None, None, None)
    assert lib.ukfb_predict_sampled_dev(None, C.byref(pin), C.c_int(1), C.byref(out)) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_predict_sampled_dev(None, C.byref(pin), C.c_int(0), C.byref(out)) == 1
    assert lib.ukfb_predict_sampled(None, buf, buf, C.c_int(0), None, C.c_int(1), None, None, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("predict_sampled_host.cpp", tmp_path)
