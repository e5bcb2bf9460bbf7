"""Pins tests/smoother_reference.py, the NumPy statement of the fixed-interval smoother (include/ukf_batch.h, "fixed-interval
smoothing"), on the CPU: the yardstick of tests/test_gpu_smooth.py must itself be right."""
import numpy as np
import pytest

import smoother_reference as sr
from engine_support import scaled

ACC_COV = 0.01 * np.eye(3)


def cpu_history(spe, onp, model, n, steps):
    """the recording of tests/test_gpu_smooth.py with the NumPy oracle as the filter -> (params, mu, cov, dt, in_a, in_b)"""
    sy = spe.synth
    dt = np.array([0.01 * (1.0 + 0.1 * c) for c in range(steps - 1)])
    mu, cov = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
    mus, covs, ia, ib = [], [], [], []
    a = b = None
    for c in range(steps):
        if model == "pose":
            acc, z, Q = sy.pose_cycle_inputs(n, c, mu[:, :3])
            acc[::5] = np.nan
            if c > 0:
                mu, cov, s1 = onp.pose_predict(mu, cov, sy.pose_default_process_noise(), a, ACC_COV, dt[c - 1])
                mu, cov, s2 = onp.pose_update(mu, cov, onp.MEAS_POS3, z, Q)
                assert not s1.any() and not s2.any()
            a, b = acc, np.zeros((n, 3))
        else:
            gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu[:, 0:4])
            if c > 0:
                mu, cov, s1 = onp.orient_predict(mu, cov, sy.orient_process_noise(), a, b, sy.ORIENT_TAU, sy.ORIENT_TAU,
                                                 onp.earth_rotation(sy.ORIENT_LATITUDE), dt[c - 1])
                mu, cov, s2 = onp.orient_update(mu, cov, z, Q)
                assert not s1.any() and not s2.any()
            a, b = acc, gyro
        mus.append(mu); covs.append(cov); ia.append(a); ib.append(b)
    if model == "pose":
        p = sr.Params("pose", sy.pose_default_process_noise(), acc_cov=ACC_COV)
    else:
        p = sr.Params("orient", sy.orient_process_noise(), tau_g=sy.ORIENT_TAU, tau_a=sy.ORIENT_TAU,
                      earth=onp.earth_rotation(sy.ORIENT_LATITUDE))
    return p, np.array(mus), np.array(covs), dt, np.array(ia), np.array(ib)


def linear_case(rot_var, B=32, steps=5, seed=3):
    """Pose, identity orientation, zero angular velocity, the acceleration branch: (p, v) is the linear system
    p' = p + dt v + dt^2 a, v' = v + dt a with the raw noise (velocity block 2 acc.cov)"""
    rng = np.random.default_rng(seed)
    mu = np.zeros((steps, B, 13)); mu[..., 6] = 1.0
    mu[..., 0:3] = rng.uniform(-5, 5, (steps, B, 3)); mu[..., 7:10] = rng.uniform(-1, 1, (steps, B, 3))
    G = rng.uniform(-1, 1, (steps, B, 6, 6))
    P6 = 0.01 * (np.eye(6) + G @ np.swapaxes(G, -1, -2) / 6.0)
    cov = np.zeros((steps, B, 12, 12))
    pv = [0, 1, 2, 6, 7, 8]
    cov[np.ix_(range(steps), range(B), pv, pv)] = P6
    for k in (3, 4, 5, 9, 10, 11):
        cov[..., k, k] = rot_var
    R = np.diag([0.01] * 3 + [rot_var] * 3 + [0.0] * 3 + [rot_var] * 3)
    acc = rng.uniform(-0.5, 0.5, (steps, B, 3))
    dt = np.array([0.02, 0.05, 0.01, 0.03])[:steps - 1]
    return sr.Params("pose", R, acc_cov=ACC_COV), mu, cov, dt, acc, pv, P6


def textbook_rts(mu, P6, dt, acc, pv):
    steps, B = mu.shape[:2]
    x = mu[..., [0, 1, 2, 7, 8, 9]]
    Q6 = np.zeros((6, 6)); Q6[:3, :3] = 0.01 * np.eye(3); Q6[3:, 3:] = 2.0 * ACC_COV
    xs, Ps = x.copy(), P6.copy()
    for c in range(steps - 2, -1, -1):
        F = np.eye(6); F[:3, 3:] = dt[c] * np.eye(3)
        u = np.concatenate([dt[c] ** 2 * acc[c], dt[c] * acc[c]], axis=-1)
        xp = x[c] @ F.T + u
        Pp = F @ P6[c] @ F.T + Q6
        Gn = P6[c] @ F.T @ np.linalg.inv(Pp)
        xs[c] = x[c] + np.einsum("bij,bj->bi", Gn, xs[c + 1] - xp)
        Ps[c] = P6[c] + Gn @ (Ps[c + 1] - Pp) @ np.swapaxes(Gn, -1, -2)
    return xs, Ps


def linear_errors(rot_var):
    p, mu, cov, dt, acc, pv, P6 = linear_case(rot_var)
    mu_s, cov_s, st, _ = sr.smooth(p, mu, cov, dt, in_a=acc)
    assert not st.any()
    xs, Ps = textbook_rts(mu, P6, dt, acc, pv)
    got_x = mu_s[..., [0, 1, 2, 7, 8, 9]]
    got_P = cov_s[np.ix_(range(mu.shape[0]), range(mu.shape[1]), pv, pv)]
    return scaled(got_x, xs), scaled(got_P, Ps)


def test_linear_known_answer():
    ex, eP = linear_errors(1e-12)
    print(f"linear known answer at rotation variance 1e-12: scaled errors mean {ex:.3e} cov {eP:.3e}")
    assert ex <= 1e-9 and eP <= 1e-9
    # What is left is the set-up's residual nonlinearity -- the rotation's spread couples into the position through R(q) v -- and
    # not luck: it is of first order in the rotation variance.  At variances where it stands six orders above rounding
    # (2.7e-7 and 5.5e-10 scaled at 1e-6) halving the variance must halve it, strictly and to within a tenth; carried down to
    # 1e-12 the same line gives the 2.7e-13 the bound above is measured against.
    big, half = linear_errors(1e-6), linear_errors(0.5e-6)
    print("residual nonlinearity at rotation variance 1e-6 / 0.5e-6 (mean, cov):", big, half)
    for b, h in zip(big, half):
        assert b > 1e-11 and h < b and 0.45 <= h / b <= 0.55, (b, h)
    assert 0.5e-6 <= big[0] / ex * 1e-12 <= 2e-6   # the residual at 1e-12 lies on that line as well


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_structure_status_and_definiteness(spe, onp, model):
    p, mu, cov, dt, ia, ib = cpu_history(spe, onp, model, 1022, 6)
    mu_s, cov_s, st, sts = sr.smooth(p, mu, cov, dt, in_a=ia, in_b=ib)
    assert not st.any() and not sts.any()
    ev = np.linalg.eigvalsh(cov_s)
    tr0, trs = np.trace(cov[0], axis1=1, axis2=2).mean(), np.trace(cov_s[0], axis1=1, axis2=2).mean()
    print(f"{model}: min eigenvalue {ev.min():.3e}, mean trace at step 0 {tr0:.4f} -> {trs:.4f}")
    assert ev.min() > 0 and trs < tr0
    assert np.array_equal(mu_s[-1], mu[-1]) and np.array_equal(cov_s[-1], cov[-1])
    # steps - 1 chained windows of 2 equal one window of steps
    m2, c2 = mu.copy(), cov.copy()
    for c in range(4, -1, -1):
        a, b, _, _ = sr.smooth(p, m2[c:c + 2], c2[c:c + 2], dt[c:c + 1], in_a=ia[c:c + 2], in_b=ib[c:c + 2])
        m2[c], c2[c] = a[0], b[0]
    assert np.array_equal(m2, mu_s) and np.array_equal(c2, cov_s)
    # a window of 2 with a gated dt returns the last step's bits
    a, b, s, _ = sr.smooth(p, mu[:2], cov[:2], np.array([0.0]), in_a=ia[:2], in_b=ib[:2])
    assert np.array_equal(a[0], mu[1]) and np.array_equal(b[0], cov[1]) and (s == onp.ST_SKIPPED_SMALL_DT).all()
    # size of the transport: the same window with J = I
    mu_i, cov_i, _, _ = sr.smooth(p, mu, cov, dt, in_a=ia, in_b=ib, transport=False)
    diff = max(scaled(mu_i, mu_s), scaled(cov_i, cov_s))
    print(f"{model}: largest scaled difference of J = I against the transport: {diff:.3e}")
    assert diff > 0.0


def test_failure_keeps_the_filtered_record(spe, onp):
    p, mu, cov, dt, ia, ib = cpu_history(spe, onp, "pose", 8, 4)
    cov = cov.copy()
    cov[2, 5] = -np.eye(12)
    mu_s, cov_s, st, sts = sr.smooth(p, mu, cov, dt, in_a=ia)
    assert st[5] == onp.ST_ERR_CHOLESKY and not np.delete(st, 5).any()
    assert np.array_equal(mu_s[2, 5], mu[2, 5]) and np.array_equal(cov_s[2, 5], cov[2, 5])
    assert sts[0, 5] == 0 or np.array_equal(mu_s[0, 5], mu[0, 5])
