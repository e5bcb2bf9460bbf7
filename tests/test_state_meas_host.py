"""The joint state-block measurements without a GPU: the symbols of include/ukf_batch.h are exported and bound, the host
decisions of ukf_host.hpp (check_state_meas_args, the masks per model, state_meas_geometry, body_state_to_measurement) hold
under ASan / UBSan (tests/cpp/state_meas_host.cpp, compiled here), and a NULL engine is refused before anything touches a
device."""
import ctypes as C

from host_support import header_text, run_sanitized

NAMES = ("ukfb_update_state_dev", "ukfb_update_state", "ukfb_pose_update_body_states")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("update_state_dev", "update_state", "update_body_states"):
        assert callable(getattr(spe.BatchUKF, method))
    assert "ukfb_state_meas_out" in header and [f[0] for f in spe.engine.StateMeasOut._fields_] == ["maha", "loglik", "status"]
    assert (spe.BLOCK_POSE_POSITION, spe.BLOCK_POSE_ORIENTATION, spe.BLOCK_POSE_VELOCITY, spe.BLOCK_POSE_ANGULAR_VELOCITY,
            spe.BLOCK_POSE_ALL) == (1, 2, 4, 8, 15)
    assert (spe.BLOCK_ORIENT_ORIENTATION, spe.BLOCK_ORIENT_VELOCITY, spe.BLOCK_ORIENT_BIAS_GYRO, spe.BLOCK_ORIENT_BIAS_ACC,
            spe.BLOCK_ORIENT_GRAVITY, spe.BLOCK_ORIENT_ALL) == (1, 2, 4, 8, 16, 31)


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    buf = (C.c_double * 512)()
    out = spe.engine.StateMeasOut(None, None, None)
    one = C.c_double(1.0)
    assert lib.ukfb_update_state_dev(None, C.c_uint32(1), None, buf, buf, one, one, C.c_int(1), C.byref(out)) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_update_state(None, C.c_uint32(1), None, buf, buf, one, one, C.c_int(1), None, None, None) == 1
    assert lib.ukfb_pose_update_body_states(None, C.c_uint32(1), buf, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    run_sanitized("state_meas_host.cpp", tmp_path)
