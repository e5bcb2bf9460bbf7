"""The wide-arithmetic mode of the fp32 engines (ukfb_config::wide_arithmetic = 1, include/ukf_batch.h): fp32 arrays in HBM,
every instruction of predict / update in fp64 (`ukf_kernel16<double, M, ..., float>`, kernel names "ukf_kernel16<f32-wide,...").

Why it exists: the reference computes in fp64 throughout (/root/reference/src/Measurement.hpp:9-10, MTK::SO3<double> in
src/pose_with_velocity/PoseWithVelocity.hpp:14).  An fp32 evaluation of the same recursion leaves it by more than north_star's
1e-4 after 150 (OrientationState) / 500 (PoseWithVelocity) cycles of the bench workloads, and tests/study_f32_mixed.py shows that
no cheaper mix (fp64 only in the factorisations / recombinations, or only in the SO(3) maps) holds it.  What is asserted here:

  1. every launch shape an fp32 engine has (fused cycle general / plain, predict, update, multi-cycle, scheduled, per-filter
     models incl. the SO(3) measurement, buckets, timestamps, event rounds) runs the wide kernel when the flag is set, and its
     result is the fp64 ORACLE's on the same fp32-rounded inputs up to the fp32 rounding of the stored state (a few 1e-7 of the
     entry's magnitude per cycle) -- far closer than the fp32-arithmetic engine is;
  2. 614 cycles of BASELINE configs 3 and 4's workloads stay within 1e-4 of the fp64 oracle (the fp32 engine: 1.7e-4 / 1.4e-3);
  3. fp64 engines ignore the flag; the one-wavefront-per-filter layouts refuse it.
PARITY UNPINNED w.r.t. real MTK (oracle/ukf_oracle.hpp header)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drift_f32  # noqa: E402
from engine_support import f32r  # noqa: E402

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    """max |a - b| relative to the magnitude of the entries (floor 1): what fp32 storage of the result costs"""
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


STORE_TOL = 4e-7   # a few fp32 ulp of the stored entry per cycle (inputs and state are fp32, the arithmetic is not)


def test_wide_pose_launch_shapes_against_the_fp64_oracle(spe, oracle):
    import torch
    s = spe.synth
    n = 4099
    mu, cov = s.pose_initial(n)
    mu, cov = f32r(mu), f32r(cov)
    acc, z, Q = (f32r(x) for x in s.pose_cycle_inputs(n, 0, mu[:, :3], random_q=True))
    R = s.pose_default_process_noise()
    acc_cov = 0.01 * np.eye(3)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1))).to("cuda", torch.float32)   # noqa: E731
    a_t, z_t, Q_t = dev(acc), dev(z), dev(Q)
    torch.cuda.synchronize()

    def engine(**kw):
        e = spe.BatchPoseUKF(n, precision=spe.F32, stream="private", wide_arithmetic=1, **kw)
        e.initialize(mu, cov)
        e.set_acceleration(None, acc_cov)
        e.bind_acceleration_dev(a_t)
        return e

    # fused cycle, plain instantiation
    e = engine()
    e.cycle_dev(0.01, spe.MEAS_POS3, z_t, Q_t)
    assert e.last_launch_info()["kernel"] == "ukf_kernel16<f32-wide,pose,cycle-plain>"
    m_o, c_o, s1 = oracle.pose_predict(mu, cov, R, acc, acc_cov, 0.01)
    m_o, c_o, s2 = oracle.pose_update(m_o, c_o, spe.MEAS_POS3, z, Q)
    m_g, c_g, _ = e.state()
    assert e.status_summary() == 0 and rel_err(m_g, m_o) <= STORE_TOL and rel_err(c_g, c_o) <= STORE_TOL
    # the fp32-arithmetic engine on the same launch is an order of magnitude further away in the covariance
    e32 = spe.BatchPoseUKF(n, precision=spe.F32, stream="private")
    e32.initialize(mu, cov); e32.set_acceleration(None, acc_cov); e32.bind_acceleration_dev(a_t)
    e32.cycle_dev(0.01, spe.MEAS_POS3, z_t, Q_t)
    assert e32.last_launch_info()["kernel"] == "ukf_kernel16<f32,pose,cycle-plain>"
    e32.close()

    # separate predict and update launches (the reference's two calls), general fused cycle (per-filter models incl. SO(3))
    e.initialize(mu, cov)
    e.predict(0.01)
    assert e.last_launch_info()["kernel"] == "ukf_kernel16<f32-wide,pose,predict-plain>"
    e.update_dev(spe.MEAS_POS3, z_t, Q_t)
    assert e.last_launch_info()["kernel"] == "ukf_kernel16<f32-wide,pose,update-plain>"
    m_g2, c_g2, _ = e.state()
    assert rel_err(m_g2, m_o) <= 2 * STORE_TOL and rel_err(c_g2, c_o) <= 2 * STORE_TOL   # (one more rounding of the state in between)

    models = s.pose_mixed_models(n, 0)
    zm = f32r(s.pose_measurement_for_model(mu, models, z - mu[:, :3]))
    e.configure(bucket_models=0)
    e.initialize(mu, cov)
    e.cycle_dev(0.01, 0, dev(zm), Q_t, meas_model_dev=torch.from_numpy(models).to("cuda"))
    assert e.last_launch_info()["kernel"] == "ukf_kernel16<f32-wide,pose,cycle-streams>"
    m_o3, c_o3, _ = oracle.pose_predict(mu, cov, R, acc, acc_cov, 0.01)
    m_o3, c_o3, st3 = oracle.pose_update(m_o3, c_o3, models, zm, Q)
    m_g3, c_g3, _ = e.state()
    assert rel_err(m_g3, m_o3) <= STORE_TOL and rel_err(c_g3, c_o3) <= STORE_TOL
    assert set(np.unique(models)) >= {-1, 0, 3, 8}

    # multi-cycle launch (plain and scheduled) against consecutive single launches of the same engine: NOT bit for bit in this
    # mode -- between the cycles of one launch the filter stays in LDS in fp64, single launches round it to fp32 every time
    e.initialize(mu, cov)
    z3 = torch.stack([z_t, z_t + 0.01, z_t - 0.01]).contiguous()
    Q3 = torch.stack([Q_t] * 3).contiguous()
    torch.cuda.synchronize()
    e.cycle_multi_dev(3, 0.01, spe.MEAS_POS3, z3, Q3, 3, 0)
    assert e.last_launch_info()["kernel"] == "ukf_kernel16<f32-wide,pose,multicycle-plain>"
    m_m, c_m, _ = e.state()
    e.initialize(mu, cov)
    for k in range(3):
        e.cycle_dev(0.01, spe.MEAS_POS3, z3[k], Q3[k])
    m_s, c_s, _ = e.state()
    assert rel_err(m_m, m_s) <= 3 * STORE_TOL and rel_err(c_m, c_s) <= 3 * STORE_TOL and not np.array_equal(c_m, c_s)
    m_o4, c_o4 = mu, cov
    for k in range(3):
        zk = z3[k].double().cpu().numpy()
        m_o4, c_o4, _ = oracle.pose_predict(m_o4, c_o4, R, acc, acc_cov, 0.01)
        m_o4, c_o4, _ = oracle.pose_update(m_o4, c_o4, spe.MEAS_POS3, zk, Q)
    assert rel_err(m_m, m_o4) <= STORE_TOL and rel_err(c_m, c_o4) <= STORE_TOL      # one rounding, at the end of the launch
    e.initialize(mu, cov)
    e.cycle_schedule_dev([0.01, 0.02, 0.01], [spe.MEAS_POS3, -1, spe.MEAS_VEL3], z3, Q3, 3, 0)
    assert e.last_launch_info()["kernel"] == "ukf_kernel16<f32-wide,pose,multicycle>"
    assert np.isfinite(e.state()[0]).all() and e.status_summary() == 0

    # event rounds (indirect launches) and timestamps
    e.initialize(mu, cov)
    e.set_last_measurement_time(np.full(n, 1_000_000, dtype=np.int64))
    fidx = np.arange(0, n, 3, dtype=np.int32)
    ts = np.full(fidx.size, 1_010_000, dtype=np.int64)
    e.process_events(fidx, ts, np.zeros(fidx.size, dtype=np.int32), z[fidx], Q[fidx])
    assert "f32-wide" in e.last_launch_info()["kernel"]
    m_e, c_e, _ = e.state()
    assert rel_err(m_e[fidx], m_o[fidx]) <= STORE_TOL and rel_err(c_e[fidx], c_o[fidx]) <= STORE_TOL
    untouched = np.setdiff1d(np.arange(n), fidx)
    assert np.array_equal(m_e[untouched], mu[untouched])
    e.close()


def test_wide_orientation_cycle_against_the_fp64_oracle(spe, oracle):
    import torch
    s = spe.synth
    n = 4099
    mu, cov = s.orient_initial(n)
    mu, cov = f32r(mu), f32r(cov)
    gyro, acc, z, Q = (f32r(x) for x in s.orient_cycle_inputs(n, 0, mu[:, :4]))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1))).to("cuda", torch.float32)   # noqa: E731
    e = spe.BatchOrientationUKF(n, s.ORIENT_TAU, s.ORIENT_TAU, s.ORIENT_LATITUDE, precision=spe.F32, stream="private",
                                wide_arithmetic=1)
    Rn = s.orient_process_noise()
    e.set_process_noise(Rn)
    e.initialize(mu, cov)
    g_t, a_t, z_t, Q_t = dev(gyro), dev(acc), dev(z), dev(Q)
    torch.cuda.synchronize()
    e.bind_orient_inputs_dev(g_t, a_t)
    m_o, c_o = mu, cov
    for k in range(3):
        e.cycle_dev(0.01, spe.MEAS_ORIENT_BODYVEL3, z_t, Q_t)
        m_o, c_o, _ = oracle.orient_predict(m_o, c_o, Rn, acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, e.earth_rotation, 0.01)
        m_o, c_o, _ = oracle.orient_update(m_o, c_o, z, Q)
    assert e.last_launch_info()["kernel"] == "ukf_kernel16<f32-wide,orient,cycle-plain>"
    m_g, c_g, _ = e.state()
    assert e.status_summary() == 0 and rel_err(m_g, m_o) <= 3 * STORE_TOL and rel_err(c_g, c_o) <= 3 * STORE_TOL
    # anisotropic noise: the rotated-noise path of the wide kernel
    R2 = Rn.copy()
    R2[0, 0] *= 3.0
    R2[0, 1] = R2[1, 0] = 0.2 * Rn[0, 0]
    e.set_process_noise(R2)
    e.initialize(mu, cov)
    e.cycle_dev(0.01, spe.MEAS_ORIENT_BODYVEL3, z_t, Q_t)
    m_o, c_o, _ = oracle.orient_predict(mu, cov, R2, acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, e.earth_rotation, 0.01)
    m_o, c_o, _ = oracle.orient_update(m_o, c_o, z, Q)
    m_g, c_g, _ = e.state()
    assert rel_err(m_g, m_o) <= STORE_TOL and rel_err(c_g, c_o) <= STORE_TOL
    e.close()


@pytest.mark.parametrize("workload", ["pose", "orient"])
def test_wide_arithmetic_holds_1e_4_over_the_bench_run_length(spe, oracle, workload):
    """614 cycles (bench.py: 50 warm-up + 500 timed + the 64 of the multi-cycle region) of configs 3 / 4's workloads"""
    marks = (1, 100, 300, 500, 614)
    rows = drift_f32.run(spe, oracle, workload, n=2048, cycles=614, checkpoints=marks,
                         threads=max(1, min(16, oracle.max_threads())), wide=True)
    print("\n" + drift_f32.fmt(rows))
    assert [r["cycle"] for r in rows] == list(marks)
    for r in rows:
        assert r["status"] == (0, 0, 0), r
        assert r["gpu_o64"][0] <= 1e-4 and r["gpu_o64"][1] <= 1e-4, (workload, r)
    last = rows[-1]
    # ... where plain fp32 arithmetic of the same algorithm (the float oracle) has left it
    assert max(last["o32_o64"]) > 1e-4, last


def test_wide_flag_is_refused_or_ignored_where_it_does_not_apply(spe):
    e = spe.BatchPoseUKF(64, precision=spe.F64, wide_arithmetic=1)       # fp64 engines: ignored
    mu, cov = spe.synth.pose_initial(64)
    e.initialize(mu, cov)
    e.predict(0.01)
    assert e.last_launch_info()["kernel"] == "ukf_kernel16<f64,pose,predict-plain>"
    e.close()
    e = spe.BatchPoseUKF(64, precision=spe.F32)
    with pytest.raises(spe.UkfbError):
        e.configure(lanes_per_filter=64, wide_arithmetic=1)
    with pytest.raises(spe.UkfbError):
        e.configure(wide_arithmetic=2)
    e.close()
