"""Dense process noise on every launch path.  The kernels fetch each lane's noise entries by offset through the lane tables
(Pose covariance phase, OrientationState phase, the shaped table of the rotated 6x6 block, the host-built acceleration-branch
table Racc) and per-filter noise at filter * D * D: with a noise whose every lower-triangle entry is nonzero and distinct
(synth.dense_process_noise*, tests/test_noise_cases.py) a misaddressed entry shows as a parity failure, where a diagonal noise
reads 0 where 0 is expected.  Against the CPU oracle at the north_star tolerances; every case asserts the kernel it ran.

Also the host condition of the short update factorisation (ukfb_config::full_update_check): a positive semidefinite noise whose
rotated blocks are coupled to other blocks can turn indefinite in the prediction (synth.rotation_indefinite_noise), so it must
keep the complete factorisation -- full_update_check 0 and 1 give the oracle's status words."""
import os

import numpy as np
import pytest

from conftest import max_abs
from engine_support import f32r

pytestmark = pytest.mark.gpu

TOL = {0: 1e-9, 1: 1e-4}  # F64, F32
THREADS = 8               # oracle threads (a GPU box command has 16 CPUs)


def _dev(x, prec):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(x.shape[0], -1))).to(
        "cuda", torch.float64 if prec == 0 else torch.float32)


def _noise(spe, model, n, kind):
    s = spe.synth
    return s.dense_process_noise_per_filter(model, n) if kind == "per_filter" else s.dense_process_noise(model)


def _set_noise(e, R):
    if R.ndim == 3:
        e.set_process_noise(R, first=0)
    else:
        e.set_process_noise(R)


def _stored(R, prec):
    """the noise the engine holds: fp32 engines round it to float"""
    return R if prec == 0 else f32r(R)


class _PoseCase:
    """One Pose batch: dense noise (batch-uniform or per filter), the constant-velocity branch (acceleration NaN), the
    acceleration branch with a dense acceleration covariance, or both mixed inside every wavefront."""

    def __init__(self, spe, oracle, n, prec, kind, branch):
        s = spe.synth
        self.spe, self.oracle, self.n, self.prec = spe, oracle, n, prec
        self.mu, self.cov = s.pose_initial(n)
        self.acc, self.z, self.Q = s.pose_cycle_inputs(n, 0, self.mu[:, :3], random_q=True)
        if branch == "cv":
            self.acc[:] = np.nan
        elif branch == "mixed":
            self.acc[1::3] = np.nan
        self.acc_cov = s.dense_acc_cov()
        self.R = _noise(spe, "pose", n, kind)
        self.Ro = _stored(self.R, prec)

    def engine(self, **kw):
        e = self.spe.BatchPoseUKF(self.n, precision=self.prec, **kw)
        _set_noise(e, self.R)
        e.initialize(self.mu, self.cov)
        e.set_acceleration(self.acc, self.acc_cov)
        return e

    def predict(self, mu, cov, dt):
        return self.oracle.pose_predict(mu, cov, self.Ro, self.acc, self.acc_cov, dt, threads=THREADS)

    def update(self, mu, cov, model, z, Q):
        return self.oracle.pose_update(mu, cov, model, z, Q, threads=THREADS)


def _check(e, m_o, c_o, st_o, prec, zero_status=True):
    m_g, c_g, init = e.state()
    st_g = e.status()
    assert init.all() and (st_g == st_o).all()
    if zero_status:
        assert (st_o == 0).all()
    assert max_abs(m_g, m_o) <= TOL[prec], max_abs(m_g, m_o)
    assert max_abs(c_g, c_o) <= TOL[prec], max_abs(c_g, c_o)


def _predict_kernel(prec, model, G):
    p = "f64" if prec == 0 else "f32"
    return f"ukf_kernel16<{p},{model},predict-plain>" if G == 16 else f"ukf_kernel<{p},{model},G{G},predict>"


def _general_kernel(fn):
    os.environ["UKFB_NO_PLAIN_KERNEL"] = "1"
    try:
        return fn()
    finally:
        os.environ.pop("UKFB_NO_PLAIN_KERNEL", None)


# ------------------------------------------------------------------------------------------------------ predict, every layout
@pytest.mark.parametrize("kind", ["uniform", "per_filter"])
@pytest.mark.parametrize("G", [16, 32, 64])
@pytest.mark.parametrize("prec", [0, 1])
def test_predict_dense_noise(spe, oracle, prec, G, kind):
    n = 203
    c = _PoseCase(spe, oracle, n, prec, kind, "mixed")
    e = c.engine(lanes_per_filter=G)
    e.predict(0.02)
    assert e.last_launch_info()["kernel"] == _predict_kernel(prec, "pose", G)
    _check(e, *c.predict(c.mu, c.cov, 0.02), prec)
    e.close()
    s = spe.synth
    mu, cov = s.orient_initial(n)
    gyro, acc, _, _ = s.orient_cycle_inputs(n, 0, mu[:, :4])
    R = _noise(spe, "orient", n, kind)
    e = spe.BatchOrientationUKF(n, s.ORIENT_TAU, s.ORIENT_TAU, s.ORIENT_LATITUDE, precision=prec, lanes_per_filter=G)
    _set_noise(e, R)
    e.initialize(mu, cov)
    e.set_orient_inputs(gyro, acc)
    e.predict(0.02)
    assert e.last_launch_info()["kernel"] == _predict_kernel(prec, "orient", G)
    _check(e, *oracle.orient_predict(mu, cov, _stored(R, prec), acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, e.earth_rotation, 0.02,
                                     threads=THREADS), prec)
    e.close()


# ------------------------------------------------------------------------------------------------------ Pose, every path
@pytest.mark.parametrize("branch", ["cv", "acc", "mixed"])
@pytest.mark.parametrize("kind", ["uniform", "per_filter"])
@pytest.mark.parametrize("prec", [0, 1])
def test_pose_paths_dense_noise(spe, oracle, prec, kind, branch):
    import torch
    n = 4099
    c = _PoseCase(spe, oracle, n, prec, kind, branch)
    dt = 0.02
    pred = c.predict(c.mu, c.cov, dt)

    def fused(model, z, Q):
        m, cv, s1 = pred
        m, cv, s2 = c.update(m, cv, model, z, Q)
        return m, cv, s1 | s2

    # separate predict() and update()
    e = c.engine()
    e.predict(dt)
    assert e.last_launch_info()["kernel"].endswith(",predict-plain>")
    _check(e, *pred, prec)
    e.update(spe.MEAS_POS3, c.z, c.Q)
    assert e.last_launch_info()["kernel"].endswith(",update-plain>")
    _check(e, *fused(spe.MEAS_POS3, c.z, c.Q), prec)
    e.close()
    # cycle(), the general kernel
    e = c.engine()
    _general_kernel(lambda: e.cycle(dt, spe.MEAS_POS3, c.z, c.Q))
    assert e.last_launch_info()["kernel"].endswith(",pose,cycle>")
    _check(e, *fused(spe.MEAS_POS3, c.z, c.Q), prec)
    e.close()
    # cycle_dev, plain and with per-filter models (streams only)
    z_t, Q_t = _dev(c.z, prec), _dev(c.Q, prec)
    models = spe.synth.pose_mixed_models(n, 0)
    zm = spe.synth.pose_measurement_for_model(c.mu, models, c.z - c.mu[:, :3])
    zm_t, m_t = _dev(zm, prec), torch.from_numpy(models).to("cuda")
    torch.cuda.synchronize()
    e = c.engine()
    e.cycle_dev(dt, spe.MEAS_POS3, z_t, Q_t)
    assert e.last_launch_info()["kernel"].endswith(",pose,cycle-plain>")
    _check(e, *fused(spe.MEAS_POS3, c.z, c.Q), prec)
    e.close()
    e = c.engine()
    e.cycle_dev(dt, 0, zm_t, Q_t, meas_model_dev=m_t)
    assert e.last_launch_info()["kernel"].endswith(",pose,cycle-streams>")
    _check(e, *fused(models, zm, c.Q), prec, zero_status=False)
    e.close()
    # three cycles in one launch against the oracle stepped three times
    z2 = np.stack([c.z, c.z + 0.01])
    Q2 = np.stack([c.Q, c.Q])
    z2_t = torch.stack([_dev(z2[0], prec), _dev(z2[1], prec)]).contiguous()
    Q2_t = torch.stack([Q_t, Q_t]).contiguous()
    torch.cuda.synchronize()
    e = c.engine()
    e.cycle_multi_dev(3, dt, spe.MEAS_POS3, z2_t, Q2_t, 2, 0)
    assert e.last_launch_info()["kernel"].endswith(",pose,multicycle-plain>")
    m, cv, st = c.mu, c.cov, np.zeros(n, dtype=np.uint32)
    for k in range(3):
        m, cv, s1 = c.predict(m, cv, dt)
        m, cv, s2 = c.update(m, cv, spe.MEAS_POS3, z2[k % 2], Q2[k % 2])
        st |= s1 | s2
    _check(e, m, cv, st, prec)
    e.close()
    # per-filter sample times: dt (constant-velocity branch: dt R) differs from filter to filter
    t0 = 5_000_000
    ts = t0 + 10_000 + 37 * (np.arange(n, dtype=np.int64) % 97)
    mod = np.where(np.arange(n) % 5 == 3, spe.MEAS_VEL3, spe.MEAS_POS3).astype(np.int32)
    zt = spe.synth.pose_measurement_for_model(c.mu, mod, c.z - c.mu[:, :3])
    e = c.engine()
    e.set_last_measurement_time(np.full(n, t0, dtype=np.int64))
    e.cycle_timestamps(ts, mod, zt, c.Q)
    assert e.last_launch_info()["kernel"].endswith(",pose,cycle>")
    _, dts, gs = oracle.gate_timestamps(ts, np.full(n, t0, dtype=np.int64))
    assert (gs == 0).all() and np.ptp(dts) > 1e-3
    m, cv, s1 = c.predict(c.mu, c.cov, dts)
    m, cv, s2 = c.update(m, cv, mod, zt, c.Q)
    _check(e, m, cv, s1 | s2, prec)
    assert (e.last_measurement_time() == ts).all()
    e.close()
    # an event stream in arbitrary order: two samples per filter
    rng = np.random.default_rng(5)
    f_ev = np.concatenate([np.arange(n), np.arange(n)])
    t_ev = np.concatenate([ts, ts + 20_000 + 13 * (np.arange(n) % 31)])
    m_ev = np.concatenate([mod, np.full(n, spe.MEAS_VEL3, dtype=np.int32)])
    z_ev = np.concatenate([zt, c.mu[:, 7:10] + 0.02])
    Q_ev = np.concatenate([c.Q, c.Q])
    perm = rng.permutation(2 * n)
    e = c.engine()
    e.set_last_measurement_time(np.full(n, t0, dtype=np.int64))
    st_or, rounds = e.process_events(f_ev[perm], t_ev[perm], m_ev[perm], z_ev[perm], Q_ev[perm])
    assert ",pose,cycle" in e.last_launch_info()["kernel"] and rounds >= 2
    m, cv, st = c.mu, c.cov, np.zeros(n, dtype=np.uint32)
    last = np.full(n, t0, dtype=np.int64)
    for k in range(2):
        sl = slice(k * n, (k + 1) * n)
        last, dts, gs = oracle.gate_timestamps(t_ev[sl], last)
        assert (gs == 0).all()
        m, cv, s1 = c.predict(m, cv, dts)
        m, cv, s2 = c.update(m, cv, m_ev[sl], z_ev[sl], Q_ev[sl])
        st |= s1 | s2
    _check(e, m, cv, st, prec)
    assert st_or == int(np.bitwise_or.reduce(st))
    e.close()


@pytest.mark.parametrize("kind", ["uniform", "per_filter"])
@pytest.mark.parametrize("prec", [0, 1])
def test_pose_bucketed_streams_dense_noise(spe, oracle, prec, kind):
    """per-filter models at a size that groups the filters by update class: the noise is fetched through the filter list"""
    import torch
    n = 20_011
    c = _PoseCase(spe, oracle, n, prec, kind, "mixed")
    models = spe.synth.pose_mixed_models(n, 0)
    zm = spe.synth.pose_measurement_for_model(c.mu, models, c.z - c.mu[:, :3])
    zm_t, Q_t, m_t = _dev(zm, prec), _dev(c.Q, prec), torch.from_numpy(models).to("cuda")
    torch.cuda.synchronize()
    e = c.engine()
    e.cycle_dev(0.02, 0, zm_t, Q_t, meas_model_dev=m_t)
    assert e.last_launch_info()["kernel"].endswith(",pose,cycle-bucketed-streams>")
    m, cv, s1 = c.predict(c.mu, c.cov, 0.02)
    m, cv, s2 = c.update(m, cv, models, zm, c.Q)
    _check(e, m, cv, s1 | s2, prec, zero_status=False)
    e.close()


# ------------------------------------------------------------------------------------------------------ OrientationState paths
@pytest.mark.parametrize("kind", ["uniform", "per_filter"])
@pytest.mark.parametrize("prec", [0, 1])
def test_orientation_paths_dense_noise(spe, oracle, prec, kind):
    import torch
    s = spe.synth
    n = 4099
    mu, cov = s.orient_initial(n)
    gyro, acc, z, Q = s.orient_cycle_inputs(n, 0, mu[:, :4])
    R = _noise(spe, "orient", n, kind)
    Ro = _stored(R, prec)
    dt = 0.02
    BV = spe.MEAS_ORIENT_BODYVEL3

    def engine():
        e = spe.BatchOrientationUKF(n, s.ORIENT_TAU, s.ORIENT_TAU, s.ORIENT_LATITUDE, precision=prec)
        _set_noise(e, R)
        e.initialize(mu, cov)
        e.set_orient_inputs(gyro, acc)
        return e

    earth = engine().earth_rotation
    predict = lambda m, c, d: oracle.orient_predict(m, c, Ro, acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, earth, d, threads=THREADS)  # noqa: E731
    update = lambda m, c, zz: oracle.orient_update(m, c, zz, Q, threads=THREADS)   # noqa: E731
    m1, c1, s1 = predict(mu, cov, dt)
    m2, c2, s2 = update(m1, c1, z)
    e = engine()
    e.predict(dt)
    assert e.last_launch_info()["kernel"].endswith(",orient,predict-plain>")
    _check(e, m1, c1, s1, prec)
    e.update(BV, z, Q)
    assert e.last_launch_info()["kernel"].endswith(",orient,update-plain>")
    _check(e, m2, c2, s1 | s2, prec)
    e.close()
    e = engine()
    _general_kernel(lambda: e.cycle(dt, BV, z, Q))
    assert e.last_launch_info()["kernel"].endswith(",orient,cycle>")
    _check(e, m2, c2, s1 | s2, prec)
    e.close()
    z_t, Q_t = _dev(z, prec), _dev(Q, prec)
    z2_t, Q2_t = torch.stack([z_t, z_t]).contiguous(), torch.stack([Q_t, Q_t]).contiguous()
    torch.cuda.synchronize()
    e = engine()
    e.cycle_dev(dt, BV, z_t, Q_t)
    assert e.last_launch_info()["kernel"].endswith(",orient,cycle-plain>")
    _check(e, m2, c2, s1 | s2, prec)
    e.close()
    e = engine()
    e.cycle_multi_dev(3, dt, BV, z2_t, Q2_t, 2, 0)
    assert e.last_launch_info()["kernel"].endswith(",orient,multicycle-plain>")
    m, c, st = mu, cov, np.zeros(n, dtype=np.uint32)
    for _ in range(3):
        m, c, a = predict(m, c, dt)
        m, c, b = update(m, c, z)
        st |= a | b
    _check(e, m, c, st, prec)
    e.close()
    t0 = 5_000_000
    ts = t0 + 20_000 + 53 * (np.arange(n, dtype=np.int64) % 89)
    e = engine()
    e.set_last_measurement_time(np.full(n, t0, dtype=np.int64))
    e.cycle_timestamps(ts, np.full(n, BV, dtype=np.int32), z, Q)
    assert e.last_launch_info()["kernel"].endswith(",orient,cycle>")
    dts = (ts - t0) / 1e6
    m, c, a = predict(mu, cov, dts)
    m, c, b = update(m, c, z)
    _check(e, m, c, a | b, prec)
    e.close()


# ------------------------------------------------------------------------------------------------------ wide arithmetic
def test_wide_arithmetic_plain_cycle_per_filter_noise(spe, oracle):
    """fp32 arrays, fp64 arithmetic: the fp64 oracle on the same fp32-rounded inputs (the noise as stored) at 1e-4"""
    import torch
    n = 4099
    s = spe.synth
    mu, cov = (f32r(x) for x in s.pose_initial(n))
    acc, z, Q = (f32r(x) for x in s.pose_cycle_inputs(n, 0, mu[:, :3], random_q=True))
    acc[2::5] = np.nan
    R = s.dense_process_noise_per_filter("pose", n)
    acc_cov = s.dense_acc_cov()
    e = spe.BatchPoseUKF(n, precision=spe.F32, wide_arithmetic=1)
    e.set_process_noise(R, first=0)
    e.initialize(mu, cov)
    e.set_acceleration(acc, acc_cov)
    z_t, Q_t = _dev(z, 1), _dev(Q, 1)
    torch.cuda.synchronize()
    e.cycle_dev(0.02, spe.MEAS_POS3, z_t, Q_t)
    assert e.last_launch_info()["kernel"] == "ukf_kernel16<f32-wide,pose,cycle-plain>"
    m, c, s1 = oracle.pose_predict(mu, cov, f32r(R), acc, f32r(acc_cov), 0.02, threads=THREADS)
    m, c, s2 = oracle.pose_update(m, c, spe.MEAS_POS3, z, Q, threads=THREADS)
    _check(e, m, c, s1 | s2, 1)
    e.close()


# ------------------------------------------------------------------------------------------------------ per-filter bookkeeping
@pytest.mark.parametrize("prec", [0, 1])
def test_per_filter_noise_sub_range_and_back_to_uniform(spe, oracle, prec):
    n, k, cnt = 4099, 1001, 1500
    c = _PoseCase(spe, oracle, n, prec, "uniform", "mixed")
    A = c.R
    stack = spe.synth.dense_process_noise_per_filter("pose", cnt, seed=spe.synth.SEED_BASE + 9)
    e = c.engine()
    e.set_process_noise(stack, first=k)
    full = np.broadcast_to(A, (n, 12, 12)).copy()
    full[k:k + cnt] = stack
    for i in (0, 3, k - 1, k, k + 1, k + 4, k + cnt - 1, k + cnt, n - 1):
        assert np.array_equal(e.process_noise(i), _stored(full[i], prec)), i
    e.predict(0.02)
    assert e.last_launch_info()["kernel"].endswith(",predict-plain>")
    m, cv, st = c.oracle.pose_predict(c.mu, c.cov, _stored(full, prec), c.acc, c.acc_cov, 0.02, threads=THREADS)
    _check(e, m, cv, st, prec)
    # a batch-uniform noise again: every filter takes it
    B = spe.synth.dense_process_noise("pose", seed=spe.synth.SEED_BASE + 10)
    e.set_process_noise(B)
    for i in (0, k, n - 1):
        assert np.array_equal(e.process_noise(i), _stored(B, prec))
    e.predict(0.03)
    m, cv, st2 = c.oracle.pose_predict(m, cv, _stored(B, prec), c.acc, c.acc_cov, 0.03, threads=THREADS)
    _check(e, m, cv, st | st2, prec)
    e.close()


@pytest.mark.parametrize("prec", [0, 1])
def test_acceleration_covariance_before_and_after_per_filter_noise(spe, oracle, prec):
    """Racc (the acceleration branch's noise, velocity block = 2 acc.cov) is rebuilt when the acceleration covariance changes and
    when the noise becomes per filter"""
    n = 203
    s = spe.synth
    c = _PoseCase(spe, oracle, n, prec, "uniform", "acc")
    C1 = s.dense_acc_cov()
    C2 = s.dense_acc_cov(seed=s.SEED_BASE + 11)
    Rp = s.dense_process_noise_per_filter("pose", n, seed=s.SEED_BASE + 12)
    e = c.engine()
    e.set_acceleration(c.acc, C1)
    e.predict(0.02)
    m, cv, st = oracle.pose_predict(c.mu, c.cov, c.Ro, c.acc, C1, 0.02, threads=THREADS)
    _check(e, m, cv, st, prec)
    e.set_process_noise(Rp, first=0)
    e.predict(0.02)
    m, cv, st = oracle.pose_predict(m, cv, _stored(Rp, prec), c.acc, C1, 0.02, threads=THREADS)
    _check(e, m, cv, st, prec)
    e.set_acceleration(None, C2)
    e.predict(0.02)
    assert e.last_launch_info()["kernel"].endswith(",predict-plain>")
    m, cv, st = oracle.pose_predict(m, cv, _stored(Rp, prec), c.acc, C2, 0.02, threads=THREADS)
    _check(e, m, cv, st, prec)
    e.close()


# ------------------------------------------------------------------------------------------------------ device group
@pytest.mark.parametrize("prec", [0, 1])
def test_two_shard_group_dense_noise_equals_one_engine(spe, prec):
    n = 4099
    s = spe.synth
    mu, cov = s.pose_initial(n)
    acc, z, Q = s.pose_cycle_inputs(n, 0, mu[:, :3])
    acc[1::3] = np.nan
    R, C = s.dense_process_noise("pose"), s.dense_acc_cov()
    one = spe.BatchPoseUKF(n, precision=prec)
    grp = spe.UKFGroup(spe.MODEL_POSE, prec, n, [0, 0])
    for x in (one, grp):
        x.set_process_noise(R)
        x.initialize(mu, cov)
        x.set_acceleration(acc, C)
        x.cycle(0.02, spe.MEAS_POS3, z, Q)
        x.predict(0.01)
        x.update(spe.MEAS_VEL3, mu[:, 7:10] + 0.01, Q)
        x.sync()
    m1, c1, _ = one.state()
    mg, cg, _ = grp.state()
    assert np.array_equal(m1, mg) and np.array_equal(c1, cg)
    assert (one.status() == grp.status()).all() and one.status_summary() == 0
    one.close()
    grp.close()


# ------------------------------------------------------------------------------------------------------ short update gate
@pytest.mark.parametrize("case", ["pose-pos3", "pose-orient_so3", "orient-bodyvel3"])
def test_short_update_gate_with_rotation_indefinite_noise(spe, oracle, onp, case):
    """A batch-uniform noise that is positive semidefinite as given but indefinite after the prediction's rotation at some
    orientations (synth.rotation_indefinite_noise): filters at such an orientation reach an indefinite Sigma' whose leading
    RT + 3 columns still factorise, which only the complete factorisation of Sigma' notices (the oracle: ST_ERR_CHOLESKY).
    full_update_check 0 and 1 must give the same bits and the oracle's status words, also in a second cycle."""
    import torch
    s = spe.synth
    n = 4099
    model = case.split("-")[0]
    rng = np.random.default_rng(17)
    bad = (np.arange(n) % 7 == 2) | ((np.arange(n) >= 64) & (np.arange(n) < 72))   # lone filters and two whole wavefronts
    ang = rng.uniform(-1.2, 1.2, n)
    qx = np.stack([np.sin(0.5 * ang), np.zeros(n), np.zeros(n), np.cos(0.5 * ang)], axis=1)   # rotations about x keep R PSD
    R = s.rotation_indefinite_noise(model)
    dt = 0.1
    if model == "pose":
        mu, cov = s.pose_initial(n)
        mu[:, 3:7] = qx
        mu[bad, 3:7] = s.ROTATION_INDEFINITE_Q
        mu[bad, 7:13] = 0.0
        mu[:, 10:13] = 0.0                        # (the orientations stay where they are)
        cov[bad] = 1e-8 * np.eye(12)
        meas = spe.MEAS_POS3 if case == "pose-pos3" else spe.MEAS_ORIENT_SO3
        z = s.pose_measurement_for_model(mu, np.full(n, meas), rng.uniform(-0.05, 0.05, (n, 3)))
        inputs = {}
    else:
        mu, cov = s.orient_initial(n)
        mu[:, 0:4] = qx
        mu[bad, 0:4] = s.ROTATION_INDEFINITE_Q
        mu[bad, 4:13] = 0.0
        cov[bad] = 1e-8 * np.eye(13)
        acc = onp.quat_rotate(onp.quat_inverse(mu[:, 0:4]), np.broadcast_to([0.0, 0.0, s.ORIENT_G], (n, 3)))
        gyro = np.zeros((n, 3))
        inputs = dict(acc=acc, gyro=gyro)
        meas = spe.MEAS_ORIENT_BODYVEL3
        z = rng.uniform(-0.05, 0.05, (n, 3))
    Q = np.broadcast_to(1e-2 * np.eye(3), (n, 3, 3)).copy()
    z_t, Q_t = _dev(z, 0), _dev(Q, 0)
    torch.cuda.synchronize()

    def run(full):
        if model == "pose":
            e = spe.BatchPoseUKF(n, full_update_check=full)
        else:
            e = spe.BatchOrientationUKF(n, s.ORIENT_TAU, s.ORIENT_TAU, s.ORIENT_LATITUDE, full_update_check=full)
        e.set_process_noise(R)
        e.initialize(mu, cov)
        if model == "orient":
            e.set_orient_inputs(inputs["gyro"], inputs["acc"])       # (after initialize, which latches the ctor's inputs)
        out = []
        for _ in range(2):
            e.cycle_dev(dt, meas, z_t, Q_t)
            m, c, _ = e.state()
            out.append((m, c, e.status().copy()))
        name = e.last_launch_info()["kernel"]
        earth = getattr(e, "earth_rotation", None)
        e.close()
        return out, name, earth

    r0, k0, earth = run(0)
    r1, k1, _ = run(1)
    assert k0 == k1 and k0.endswith(",cycle-streams>" if meas == spe.MEAS_ORIENT_SO3 else ",cycle-plain>")
    m, c = mu, cov
    for cyc in range(2):
        if model == "pose":
            m, c, s1 = oracle.pose_predict(m, c, R, None, None, dt, threads=THREADS)
            m, c, s2 = oracle.pose_update(m, c, meas, z, Q, threads=THREADS)
        else:
            m, c, s1 = oracle.orient_predict(m, c, R, inputs["acc"], inputs["gyro"], s.ORIENT_TAU, s.ORIENT_TAU, earth, dt,
                                             threads=THREADS)
            m, c, s2 = oracle.orient_update(m, c, z, Q, threads=THREADS)
        st_o = s1 | s2
        (m0, c0, st0), (m1, c1, st1) = r0[cyc], r1[cyc]
        assert (st0 == st1).all(), f"cycle {cyc}: full_update_check 0 / 1 status words differ at {np.nonzero(st0 != st1)[0][:8]}"
        assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
        assert (st0 == st_o).all(), f"cycle {cyc}: status differs from the oracle at {np.nonzero(st0 != st_o)[0][:8]}"
        assert (st_o[bad] & spe.ST_ERR_CHOLESKY).all() and (st_o[~bad] == 0).all()
        assert max_abs(m0, m) <= TOL[0] and max_abs(c0, c) <= TOL[0]
