"""The user-defined measurement models without a GPU: the symbols of include/ukf_batch.h are exported and bound, the host
decisions of ukf_host.hpp (check_sampled_args, check_sigma_points_args, the range of m, the LDS accounting and launch geometry
of both kernels) hold under ASan / UBSan (tests/cpp/sampled_host.cpp, compiled here as a stand-alone program), and a NULL
engine is refused before anything touches a device."""
import ctypes as C
import os

from host_support import header_text, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_sigma_points_dev", "ukfb_update_sampled_dev", "ukfb_sigma_points", "ukfb_update_sampled")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("sigma_points_dev", "update_sampled_dev", "sigma_points", "update_sampled"):
        assert callable(getattr(spe.BatchUKF, method))
    assert "ukfb_sampled_in" in header and "ukfb_sampled_out" in header
    assert [f[0] for f in spe.SampledIn._fields_] == ["m", "Z_dev", "z_dev", "Q_dev", "q_is_uniform", "active_dev"]
    assert [f[0] for f in spe.SampledOut._fields_] == ["z_pred", "S", "innov", "maha", "loglik", "status"]
    assert C.sizeof(spe.SampledIn) == 8 + 3 * 8 + 8 + 8 and C.sizeof(spe.SampledOut) == 6 * 8
    assert spe.SAMPLED_MAX_M == 6 and "#define UKFB_SAMPLED_MAX_M 6" in header
    batch = open(os.path.join(ROOT, "include", "pose_estimation", "Batch.hpp")).read()
    assert "sigmaPoints(" in batch and "integrateSampledMeasurement(" in batch
    assert "ukfb_sigma_points(" in batch and "ukfb_update_sampled(" in batch


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    buf = (C.c_double * 64)()
    addr = C.addressof(buf)
    sin = spe.SampledIn(3, addr, addr, addr, 0, None)
    out = spe.SampledOut(None, None, None, None, None, None)
    assert lib.ukfb_sigma_points_dev(None, C.c_void_p(addr), None, None) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_update_sampled_dev(None, C.byref(sin), C.c_int(1), C.byref(out)) == 1
    assert lib.ukfb_sigma_points(None, buf, None, None) == 1
    assert lib.ukfb_update_sampled(None, C.c_int(3), buf, buf, buf, C.c_int(0), None, C.c_int(1), None, None, None, None, None,
                                   None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("sampled_host.cpp", tmp_path)
