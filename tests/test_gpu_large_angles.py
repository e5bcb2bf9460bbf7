"""Large rotations through every engine instantiation that has a wide-angle path: fast spin (|omega| dt up to ~7 rad, beyond the
2 pi reduction of cos_sinc_fast), orientation sigma ~0.5 rad (the half-angle steps of the fast logs, so3_log_fast_n2 in the fp32
kernels, the MTK log of the one-wavefront-per-filter kernel) and, for Pose, orientation measurements (MEAS_ORIENT_SO3) up to
2.5 rad away from the predicted mean.  One filter in four keeps small angles, so every wavefront (four filters on the 16-lane
layout) mixes both regimes.  The construction is the one of test_gpu_parity.py::test_large_rotations_take_the_fallback_paths,
which covers Pose in fp64 on separate predict / update launches only.

Measurements keep |z| <= pi - 0.1: near pi the plus/minus periodic log flips sign on a rounding, and engine and oracle may then
legitimately land on opposite sides.  Spreads of this size make the UKF itself ill-conditioned (the iterated mean may hit its
cap), so every case asserts the oracle's status words as well as the kernel it ran, and values against the fp64 oracle:
fp64 1e-8 (prediction) / 1e-7 (after an update) in the mean and the same times max(1, max|cov|) in the covariance; fp32
1e-4 times that scale in both.  The observed maxima on the MI355X are in each test's docstring."""
import numpy as np
import pytest

from conftest import max_abs

pytestmark = pytest.mark.gpu

N = 256
DT = 0.1
THREADS = 8
# name: (precision, engine configuration, kernel name prefix)
POSE_CFG = {
    "f64": (0, {}, "ukf_kernel16<f64,pose,"),
    "f32": (1, {}, "ukf_kernel16<f32,pose,"),                                # so3_log_fast_n2 in the mean iteration
    "f32-wide": (1, {"wide_arithmetic": 1}, "ukf_kernel16<f32-wide,pose,"),
    "f32-G64": (1, {"lanes_per_filter": 64}, "ukf_kernel<f32,pose,G64,"),    # the generic kernel: MTK's so3_exp / so3_log
}
# the kernel each launch runs: the 16-lane layout (SO(3) updates take the per-filter-model "streams" instantiations) and the
# one-wavefront-per-filter layout (no multi-cycle kernel: one cycle launch per cycle)
POSE_MODE = {16: {"predict": "predict-plain>", "update": "update-streams>", "cycle": "cycle-streams>", "cycle_multi": "multicycle>"},
             64: {"predict": "predict>", "update": "update>", "cycle": "cycle>", "cycle_multi": "cycle>"}}
ORIENT_CFG = {
    "f64": (0, {}, "ukf_kernel16<f64,orient,"),
    "f32": (1, {}, "ukf_kernel16<f32,orient,"),
    "f32-wide": (1, {"wide_arithmetic": 1}, "ukf_kernel16<f32-wide,orient,"),
}


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def so3_measurements(oracle, mu_q, big, rng):
    """z = log(q exp(delta)) with |delta| up to 2.5 rad for the wide filters (0.025 for the others) and |z| <= pi - 0.1"""
    z = np.zeros((mu_q.shape[0], 3))
    for i in range(mu_q.shape[0]):
        while True:
            d = rng.normal(size=3)
            d *= (rng.uniform(0.5, 2.5) if big[i] else rng.uniform(0.0, 0.025)) / np.linalg.norm(d)
            zi = oracle.so3_log(_qmul(mu_q[i] / np.linalg.norm(mu_q[i]), oracle.so3_exp(d)))
            if np.linalg.norm(zi) <= np.pi - 0.1:
                z[i] = zi
                break
    return z


def pose_start(spe, n=N, seed=12):
    rng = np.random.default_rng(seed)
    mu, cov = spe.synth.pose_initial(n)
    big = np.arange(n) % 4 != 0
    mu[big, 10:13] = rng.uniform(-40.0, 40.0, (int(big.sum()), 3))          # angular velocity, rad/s: |omega| dt up to ~7 rad
    for i in np.nonzero(big)[0]:
        cov[i, 3:6, :] *= 10.0
        cov[i, :, 3:6] *= 10.0                                              # orientation sigma 0.05 -> 0.5 rad
    return mu, cov, big, rng


def pose_oracle_run(spe, oracle, mu, cov, big, rng, cycles, prec=0, zs=None):
    """the oracle stepped `cycles` times (predict, then an SO(3) update drawn around the predicted orientation, or zs[k]);
    returns the measurements, the predicted state of the first cycle and the final state"""
    R = spe.synth.pose_default_process_noise()
    Q = np.stack([np.eye(3) * 0.04] * mu.shape[0])
    given, zs, st = zs, [], np.zeros(mu.shape[0], dtype=np.uint32)
    m, c = mu, cov
    pred = None
    for k in range(cycles):
        m, c, s1 = oracle.pose_predict(m, c, R, None, None, DT, prec=prec, threads=THREADS)
        st |= s1
        if pred is None:
            pred = (m, c, st.copy())
        z = so3_measurements(oracle, m[:, 3:7], big, rng) if given is None else given[k]
        zs.append(z)
        m, c, s2 = oracle.pose_update(m, c, spe.MEAS_ORIENT_SO3, z, Q, prec=prec, threads=THREADS)
        st |= s2
    return np.stack(zs), Q, pred, (m, c, st)


def _err(e, ref, prec, after_update):
    """(mean error, covariance error, bound of each) against the oracle state ref = (mu, cov, status)"""
    m_g, c_g, init = e.state()
    assert init.all()
    assert (e.status() == ref[2]).all(), (np.nonzero(e.status() != ref[2])[0][:8], e.status()[:8], ref[2][:8])
    scale = max(1.0, float(np.abs(ref[1]).max()))
    tol = (1e-7 if after_update else 1e-8) if prec == 0 else 1e-4
    return max_abs(m_g, ref[0]), max_abs(c_g, ref[1]), (tol if prec == 0 else tol * scale), tol * scale


def _kernel(e, want):
    k = e.last_launch_info()["kernel"]
    assert k == want, (k, want)
    return k


def run_pose(spe, oracle, cfg, launch):
    """one Pose case: returns [(kernel, mean error, cov error, mean bound, cov bound)] for every state compared"""
    prec, kw, prefix = POSE_CFG[cfg]
    mode = POSE_MODE[kw.get("lanes_per_filter", 16)]
    mu, cov, big, rng = pose_start(spe)
    cycles = 4 if launch == "cycle_multi" else 1
    zs, Q, pred, final = pose_oracle_run(spe, oracle, mu, cov, big, rng, cycles)
    e = spe.BatchPoseUKF(N, precision=prec, **kw)
    e.initialize(mu, cov)
    out = []
    if launch == "predict+update":
        e.predict(DT)
        k = _kernel(e, prefix + mode["predict"])
        out.append((k,) + _err(e, pred, prec, False))
        e.update(spe.MEAS_ORIENT_SO3, zs[0], Q)
        k = _kernel(e, prefix + mode["update"])
    elif launch == "cycle":
        e.cycle(DT, spe.MEAS_ORIENT_SO3, zs[0], Q)
        k = _kernel(e, prefix + mode["cycle"])
    else:
        e.cycle_multi(DT, spe.MEAS_ORIENT_SO3, zs, np.stack([Q] * cycles))
        k = _kernel(e, prefix + mode["cycle_multi"])
    out.append((k,) + _err(e, final, prec, True))
    e.close()
    return out


def orient_start(spe, n=N, seed=21):
    s = spe.synth
    rng = np.random.default_rng(seed)
    mu, cov = s.orient_initial(n)
    big = np.arange(n) % 4 != 0
    for i in np.nonzero(big)[0]:
        cov[i, 0:3, :] *= 10.0
        cov[i, :, 0:3] *= 10.0                                              # orientation sigma 0.05 -> 0.5 rad
    gyro, acc, z, Q = s.orient_cycle_inputs(n, 0, mu[:, :4])
    gyro[big] = rng.uniform(-40.0, 40.0, (int(big.sum()), 3))              # rad/s
    return mu, cov, gyro, acc, z, Q


def run_orient(spe, oracle, cfg):
    s = spe.synth
    prec, kw, prefix = ORIENT_CFG[cfg]
    mu, cov, gyro, acc, z, Q = orient_start(spe)
    R = s.orient_process_noise()
    e = spe.BatchOrientationUKF(N, s.ORIENT_TAU, s.ORIENT_TAU, s.ORIENT_LATITUDE, precision=prec, **kw)
    e.set_process_noise(R)
    e.initialize(mu, cov)
    e.set_orient_inputs(gyro, acc)
    e.cycle(DT, spe.MEAS_ORIENT_BODYVEL3, z, Q)
    k = _kernel(e, prefix + "cycle-plain>")
    m, c, s1 = oracle.orient_predict(mu, cov, R, acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, e.earth_rotation, DT, threads=THREADS)
    m, c, s2 = oracle.orient_update(m, c, z, Q, threads=THREADS)
    out = [(k,) + _err(e, (m, c, s1 | s2), prec, True)]
    e.close()
    return out


def _check(rows):
    for k, em, ec, tm, tc in rows:
        assert em <= tm and ec <= tc, (k, em, tm, ec, tc)


@pytest.mark.parametrize("launch", ["predict+update", "cycle", "cycle_multi"])
@pytest.mark.parametrize("cfg", list(POSE_CFG))
def test_pose_large_angles(spe, oracle, cfg, launch):
    """Observed on the MI355X, largest mean / covariance error against the fp64 oracle (bounds: module docstring; the
    covariance scale max(1, max|cov|) is 2.3 after the prediction, 1 after an update):

                 predict (of predict+update)   update / cycle       cycle_multi (4 cycles)
      f64        3.3e-15 / 1.1e-14             2.1e-14 / 6.0e-15    1.6e-13 / 2.0e-15
      f32        1.9e-6  / 1.5e-6              3.7e-6  / 1.4e-6     8.5e-6  / 4.1e-7
      f32-wide   1.9e-6  / 2.7e-7              3.7e-6  / 3.3e-9     3.3e-6  / 1.5e-8
      f32-G64    1.9e-6  / 3.3e-6              9.4e-6  / 1.5e-6     3.4e-5  / 1.0e-6

    The float oracle (prec=1) on the same launches is 1.1e-5 / 2.6e-6 (one cycle) and 6.6e-5 / 1.0e-6 (four cycles) away
    from the fp64 oracle: every fp32 case is within what fp32 arithmetic allows, none needed scaling back."""
    _check(run_pose(spe, oracle, cfg, launch))


@pytest.mark.parametrize("cfg", list(ORIENT_CFG))
def test_orientation_large_angles(spe, oracle, cfg):
    """Gyro rates up to +-40 rad/s, fused cycle with MEAS_ORIENT_BODYVEL3.  Observed on the MI355X (mean / covariance):
    f64 1.8e-14 / 9.8e-15, f32 3.3e-6 / 3.4e-6, f32-wide 8.9e-7 / 4.4e-7 (covariance scale 2.1)."""
    _check(run_orient(spe, oracle, cfg))


def run_neighbours(spe, oracle, prec):
    """ordinary filters alone (four per wavefront) and interleaved one per wavefront with three wide-angle filters; returns the
    largest differences of the ordinary filters' means and covariances between the two runs"""
    mu, cov, big, rng = pose_start(spe, n=4 * 64, seed=33)
    zs, Q, _, _ = pose_oracle_run(spe, oracle, mu, cov, big, rng, 1)
    ordinary = ~big
    res = []
    for sel in (ordinary, np.ones(mu.shape[0], dtype=bool)):
        n = int(sel.sum())
        e = spe.BatchPoseUKF(n, precision=prec)
        e.initialize(mu[sel], cov[sel])
        e.cycle(DT, spe.MEAS_ORIENT_SO3, zs[0][sel], Q[sel])
        m, c, _ = e.state()
        st = e.status()
        e.close()
        keep = ordinary[sel]
        res.append((m[keep], c[keep], st[keep]))
    (m1, c1, s1), (m2, c2, s2) = res
    assert (s1 == s2).all()
    return max_abs(m1, m2), max_abs(c1, c2)


@pytest.mark.parametrize("prec", [0, 1])
def test_ordinary_filters_do_not_see_wide_neighbours(spe, oracle, prec):
    """The same ordinary filters alone and sharing every wavefront with three wide-angle filters: the wide paths run behind
    wave votes, and the ordinary filters' results must not move beyond rounding (the rebase vote of the mean iteration,
    wave_all in ukf_kernel16.hpp, is per wavefront, so bit-identity is not required).  Observed on the MI355X (mean /
    covariance): fp64 5.6e-17 / 9.5e-18, fp32 3.0e-8 / 3.3e-9."""
    dm, dc = run_neighbours(spe, oracle, prec)
    tol = 1e-12 if prec == 0 else 1e-5
    assert dm <= tol and dc <= tol, (dm, dc)
