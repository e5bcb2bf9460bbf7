"""The innovation-statistics entry points without a GPU: the symbols of include/ukf_batch.h are exported with signatures that
ctypes can bind, the argument checks of ukf_host.hpp (check_innovation_args, check_select_args) hold under ASan / UBSan
(tests/cpp/innovation_host.cpp, compiled here), and a NULL engine is refused before anything touches a device."""
import ctypes as C

from host_support import run_sanitized


def test_symbols_and_signatures(spe):
    lib = spe.load_library()
    for name in ("ukfb_innovation_dev", "ukfb_select_candidates_dev", "ukfb_innovation"):
        assert name in spe.engine.EXPORTS and hasattr(lib, name)
    assert [f[0] for f in spe.engine.InnovationOut._fields_] == ["z_pred", "S", "innov", "maha", "loglik", "best", "status"]
    assert C.sizeof(spe.engine.InnovationOut) == 7 * C.sizeof(C.c_void_p)
    for method in ("innovation_dev", "select_candidates_dev", "innovation"):
        assert callable(getattr(spe.BatchUKF, method))


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    out = spe.engine.InnovationOut()
    z = (C.c_double * 3)(); Q = (C.c_double * 9)(); maha = (C.c_double * 1)()
    assert lib.ukfb_innovation(None, C.c_int(0), C.c_int(1), z, Q, None, None, None, maha, None, None, None) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_innovation_dev(None, C.c_int(0), None, C.c_int(1), z, Q, C.c_int(0), C.byref(out)) == 1
    assert lib.ukfb_select_candidates_dev(None, C.c_int(1), None, C.c_int(0), None, z, z, None) == 1


def test_argument_checks_under_sanitizers(tmp_path):
    run_sanitized("innovation_host.cpp", tmp_path)
