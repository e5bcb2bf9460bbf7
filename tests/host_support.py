"""Support for the CPU tests of the host logic: the one sanitizer build-and-run of a stand-alone program of tests/cpp, and the
text of the C header.  The programs carry statically linked ASan / UBSan runtimes; nothing is loaded into Python under a
sanitizer."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SANITIZER_MARKERS = ("AddressSanitizer", "LeakSanitizer", "runtime error", "UndefinedBehaviorSanitizer")


def header_text():
    return open(os.path.join(ROOT, "include", "ukf_batch.h")).read()


def assert_clean_run(out):
    """A finished program of tests/cpp (subprocess.CompletedProcess with captured text): it exited with 0, closed with
    expect.hpp's line for no failure, and no sanitizer spoke."""
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK: 0 failure(s)" in out.stdout
    for marker in SANITIZER_MARKERS:
        assert marker not in out.stderr + out.stdout, out.stderr


def build_sanitized(source_name, tmp_path, extra_flags=()):
    """Compile tests/cpp/<source_name> (or an absolute path) with g++ under ASan / UBSan into tmp_path; the program's path.
    extra_flags: further compiler arguments, for a program that needs more than the project's own headers."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host-side checks"
    exe = tmp_path / (os.path.splitext(os.path.basename(source_name))[0] + "_asan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    *extra_flags, os.path.join(CPP, source_name), "-o", str(exe)], check=True, timeout=300)
    return exe


def run_built(exe, args=()):
    return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=120)


def run_sanitized(source_name, tmp_path, args=(), extra_flags=()):
    """Build tests/cpp/<source_name> under the sanitizers, run it with `args` and hold the run to assert_clean_run."""
    out = run_built(build_sanitized(source_name, tmp_path, extra_flags), args)
    assert_clean_run(out)
    return out
