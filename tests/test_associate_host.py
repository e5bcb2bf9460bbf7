"""The sensor-frame association without a GPU: the symbols of include/ukf_batch.h are exported and bound, the two structures
have the C sizes, the methods of Batch.hpp and both batch classes exist, the host decisions of ukf_host.hpp
(check_associate_args, the output shapes) hold under ASan / UBSan (tests/cpp/associate_host.cpp, compiled here as a stand-alone
program), and every argument error is reported against a NULL engine before anything touches a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

from host_support import header_text, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_associate_sensor_dev", "ukfb_associate_sensor")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for cls in (spe.BatchUKF, spe.BatchPoseUKF, spe.BatchOrientationUKF):
        for method in ("associate_sensor_dev", "associate_sensor"):
            assert callable(getattr(cls, method))
    assert re.search(r"#define UKFB_ASSOCIATE_MAX_CANDIDATES 32\b", header) and spe.engine.ASSOCIATE_MAX_CANDIDATES == 32
    # the section stands after the measurements whose models and conventions it uses
    assert header.index("sensor-frame measurements: lever arms") < header.index("sensor-frame association: K candidates")
    assert header.index("ukfb_associate_out;") < header.index("user-defined measurement models: sigma-point export")
    batch = open(os.path.join(ROOT, "include", "pose_estimation", "Batch.hpp")).read()
    assert "associateSensorMeasurementDev(int model_uniform, const ukfb_associate_in& in, bool commit = true" in batch
    assert "associateSensorMeasurement(" in batch and "ukfb_associate_sensor(" in batch and "ukfb_associate_sensor_dev(" in batch
    tool = open(os.path.join(ROOT, "tools", "check_resources.py")).read()
    assert tool.count("ukf_associate_kernel") >= 2  # gated, and held to its two wavefronts per SIMD


def test_structure_sizes_match_the_header(spe, tmp_path):
    """sizeof and the field offsets of ukfb_associate_in / ukfb_associate_out as a C99 compiler lays them out"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    src = tmp_path / "sizes.c"
    fields_in = [f[0] for f in spe.AssociateIn._fields_]
    fields_out = [f[0] for f in spe.AssociateOut._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ukf_batch.h"', 'int main(void) {',
             '  printf("%zu %zu\\n", sizeof(ukfb_associate_in), sizeof(ukfb_associate_out));']
    lines += [f'  printf("%zu\\n", offsetof(ukfb_associate_in, {f}));' for f in fields_in]
    lines += [f'  printf("%zu\\n", offsetof(ukfb_associate_out, {f}));' for f in fields_out]
    lines += ['  return 0; }']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, timeout=120)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(out[0]), int(out[1])] == [C.sizeof(spe.AssociateIn), C.sizeof(spe.AssociateOut)]
    want = [getattr(spe.AssociateIn, f).offset for f in fields_in] + [getattr(spe.AssociateOut, f).offset for f in fields_out]
    assert [int(v) for v in out[2:]] == want


def test_argument_errors_against_a_null_engine(spe):
    lib = spe.load_library()
    buf = (C.c_double * 64)()
    addr = C.addressof(buf)
    mount, point = (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1), (C.c_double * 3)(1, 0, 0)
    out = spe.AssociateOut(None, None, None, addr, None, None, None, None)
    # a NULL engine is refused first, whatever else is wrong: candidates in and out of range, both modes, NULL arrays
    for K in (0, 1, 4, 32, 33):
        for hyp in (0, 1):
            for z in (addr, None):
                ain = spe.AssociateIn(None, K, z, addr, 0, None, mount, addr if hyp else None, point, hyp)
                for commit in (0, 1):
                    rc = lib.ukfb_associate_sensor_dev(None, C.c_int(0), C.byref(ain), C.c_int(commit), C.byref(out))
                    assert rc == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_associate_sensor_dev(None, C.c_int(0), None, C.c_int(1), None) == 1
    pd = C.POINTER(C.c_double)
    z = C.cast(buf, pd)
    for K in (0, 4, 33):
        assert lib.ukfb_associate_sensor(None, C.c_int(0), None, C.c_int(K), z, z, None, None, None, None, C.c_int(0), C.c_int(1), None, None,
                                         None, z, None, None, None, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("associate_host.cpp", tmp_path)
