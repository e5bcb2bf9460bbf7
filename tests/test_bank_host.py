"""The filter-bank entry points without a GPU: the symbols of include/ukf_batch.h are exported and bound, the host decisions of
ukf_host.hpp (check_bank_args, check_bank_transition, bank_geometry) hold under ASan / UBSan (tests/cpp/bank_host.cpp, compiled
here), and a NULL engine is refused before anything touches a device."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_bank_weights_dev", "ukfb_bank_combine_dev", "ukfb_bank_mix_dev", "ukfb_bank_combine", "ukfb_bank_mix")


def test_symbols_bindings_and_status_bit(spe):
    lib = spe.load_library()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name)
    for method in ("bank_weights_dev", "bank_combine_dev", "bank_mix_dev", "bank_combine", "bank_mix"):
        assert callable(getattr(spe.BatchUKF, method))
    assert spe.ST_ERR_WEIGHTS == 1 << 10
    assert "UKFB_ST_ERR_WEIGHTS = 1u << 10" in open(os.path.join(ROOT, "include", "ukf_batch.h")).read()


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    w = (C.c_double * 4)(0.5, 0.5, 0.5, 0.5); P = (C.c_double * 4)(1, 0, 0, 1); out = (C.c_double * 64)()
    assert lib.ukfb_bank_weights_dev(None, C.c_int(2), None, None, out, None, None) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_bank_combine_dev(None, C.c_int(2), w, out, None, None) == 1
    assert lib.ukfb_bank_mix_dev(None, C.c_int(2), w, P, out, None) == 1
    assert lib.ukfb_bank_combine(None, C.c_int(2), w, out, None, None) == 1
    assert lib.ukfb_bank_mix(None, C.c_int(2), w, P, out, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host-side checks"
    exe = tmp_path / "bank_host_asan"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "bank_host.cpp"), "-o", str(exe)], check=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK: 0 failure(s)" in out.stdout
    for marker in ("AddressSanitizer", "LeakSanitizer", "runtime error", "UndefinedBehaviorSanitizer"):
        assert marker not in out.stderr + out.stdout, out.stderr
