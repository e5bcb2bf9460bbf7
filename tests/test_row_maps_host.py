"""The LDS maps of the row-layout kernels without a GPU: every *_map of ukf_host.hpp lists its regions in ascending order
without overlap, keeps its aliases inside the table they alias and sums to the pinned totals, under ASan / UBSan
(tests/cpp/row_maps_host.cpp, compiled here as a stand-alone program)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_maps_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host-side checks"
    exe = tmp_path / "row_maps_host_asan"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "row_maps_host.cpp"), "-o", str(exe)], check=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK: 0 failure(s)" in out.stdout
    for marker in ("AddressSanitizer", "LeakSanitizer", "runtime error", "UndefinedBehaviorSanitizer"):
        assert marker not in out.stderr + out.stdout, out.stderr
