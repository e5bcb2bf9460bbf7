"""The support layer the other tests rest on, on the CPU: the sanitizer runner of tests/host_support.py with tests/cpp/expect.hpp
(a failed EXPECT must fail the run in every way the runner looks at), and pack / unpack / scaled of tests/engine_support.py."""
import os

import numpy as np
import pytest

from engine_support import pack, scaled, unpack
from host_support import CPP, assert_clean_run, build_sanitized, run_built

PROGRAM = '#include "%s"\nint main() {\n    EXPECT(1 + 1 == %d);\n    return finish();\n}\n'


def run_program(tmp_path, name, two):
    src = tmp_path / (name + ".cpp")
    src.write_text(PROGRAM % (os.path.join(CPP, "expect.hpp"), two))
    return run_built(build_sanitized(str(src), tmp_path))


def test_a_false_expect_fails_the_run(tmp_path):
    out = run_program(tmp_path, "fails", 3)
    assert out.returncode == 1
    assert "FAILED: 1 failure(s)" in out.stdout and "OK:" not in out.stdout + out.stderr
    assert "FAIL " in out.stdout and "1 + 1 == 3" in out.stdout   # the check that failed is named
    with pytest.raises(AssertionError):
        assert_clean_run(out)


def test_a_true_expect_passes_the_runner(tmp_path):
    out = run_program(tmp_path, "passes", 2)
    assert out.returncode == 0 and out.stdout == "OK: 0 failure(s)\n"
    assert_clean_run(out)


def test_pack_and_unpack_are_inverse_bit_for_bit():
    A = np.random.default_rng(1).standard_normal((3, 2, 12, 12))
    M = A + np.swapaxes(A, -1, -2)
    assert np.array_equal(M, np.swapaxes(M, -1, -2))
    p = pack(M)
    assert p.shape == (3, 2, 78) and p.flags["C_CONTIGUOUS"]
    assert np.array_equal(unpack(p, 12).view(np.uint64), M.view(np.uint64))


def test_pack_orders_row_r_at_r_r_plus_1_over_2():
    """pack_lower of ukf_host.hpp: (r, c), c <= r, at r (r + 1) / 2 + c"""
    M = np.array([[1.0, 2.0, 4.0], [2.0, 3.0, 5.0], [4.0, 5.0, 6.0]])
    assert pack(M).tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert np.array_equal(unpack(np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), 3), M)


def test_scaled_propagates_nan_and_takes_empty_arrays():
    x = np.array([1.0, np.nan, 3.0])
    assert np.isnan(scaled(x, np.ones(3))) and np.isnan(scaled(np.ones(3), x))
    assert not scaled(x, np.ones(3)) <= 1e300   # a NaN fails every bound
    assert scaled(np.zeros((0, 3)), np.zeros((0, 3))) == 0.0
    assert scaled(np.array([2.0, 1.0]), np.array([1.0, 1.0])) == 0.5
