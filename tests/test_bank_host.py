"""The filter-bank entry points without a GPU: the symbols of include/ukf_batch.h are exported and bound, the host decisions of
ukf_host.hpp (check_bank_args, check_bank_transition, bank_geometry) hold under ASan / UBSan (tests/cpp/bank_host.cpp, compiled
here), and a NULL engine is refused before anything touches a device."""
import ctypes as C

from host_support import header_text, run_sanitized

NAMES = ("ukfb_bank_weights_dev", "ukfb_bank_combine_dev", "ukfb_bank_mix_dev", "ukfb_bank_combine", "ukfb_bank_mix")


def test_symbols_bindings_and_status_bit(spe):
    lib = spe.load_library()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name)
    for method in ("bank_weights_dev", "bank_combine_dev", "bank_mix_dev", "bank_combine", "bank_mix"):
        assert callable(getattr(spe.BatchUKF, method))
    assert spe.ST_ERR_WEIGHTS == 1 << 10
    assert "UKFB_ST_ERR_WEIGHTS = 1u << 10" in header_text()


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    w = (C.c_double * 4)(0.5, 0.5, 0.5, 0.5); P = (C.c_double * 4)(1, 0, 0, 1); out = (C.c_double * 64)()
    assert lib.ukfb_bank_weights_dev(None, C.c_int(2), None, None, out, None, None) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_bank_combine_dev(None, C.c_int(2), w, out, None, None) == 1
    assert lib.ukfb_bank_mix_dev(None, C.c_int(2), w, P, out, None) == 1
    assert lib.ukfb_bank_combine(None, C.c_int(2), w, out, None, None) == 1
    assert lib.ukfb_bank_mix(None, C.c_int(2), w, P, out, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("bank_host.cpp", tmp_path)
