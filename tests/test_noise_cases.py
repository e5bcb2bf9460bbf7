"""CPU checks of the dense process-noise fixtures of synth.py (tests/test_gpu_process_noise.py runs them on the engine):
the two oracles agree on them, they can tell a kernel that reads the right noise entries from one that does not, and the
rotation-indefinite construction is what it claims to be."""
import numpy as np
import pytest

from conftest import max_abs

TOL_F32 = 1e-4          # the fp32 parity tolerance of the GPU tests
DT = 0.03


def _pose_inputs(spe, n, seed):
    s = spe.synth
    mu, cov = s.pose_initial(n, seed=seed)
    acc, _, _ = s.pose_cycle_inputs(n, 0, mu[:, :3], seed=seed)
    return mu, cov, acc


@pytest.mark.parametrize("per_filter", [False, True])
@pytest.mark.parametrize("branch", ["cv", "acc", "mixed"])
def test_oracles_agree_on_dense_pose_noise(spe, oracle, onp, branch, per_filter):
    n = 37
    s = spe.synth
    mu, cov, acc = _pose_inputs(spe, n, 91)
    R = s.dense_process_noise_per_filter("pose", n) if per_filter else s.dense_process_noise("pose")
    acc_cov = s.dense_acc_cov()
    if branch == "cv":
        acc = None
    elif branch == "mixed":
        acc[1::3] = np.nan
    m1, c1, s1 = oracle.pose_predict(mu, cov, R, acc, acc_cov, DT)
    m2, c2, s2 = onp.pose_predict(mu, cov, R, acc, acc_cov, DT)
    assert (s1 == 0).all() and (s2 == 0).all()
    assert max_abs(m1, m2) < 1e-12 and max_abs(c1, c2) < 1e-12
    # the predicted covariance moved by the noise well beyond the fp32 tolerance
    m0, c0, _ = onp.pose_predict(mu, cov, np.zeros((12, 12)), acc, np.zeros((3, 3)), DT)
    assert max_abs(c1, c0) > 100 * TOL_F32


@pytest.mark.parametrize("per_filter", [False, True])
def test_oracles_agree_on_dense_orientation_noise(spe, oracle, onp, per_filter):
    n = 29
    s = spe.synth
    mu, cov = s.orient_initial(n, seed=92)
    gyro, acc, _, _ = s.orient_cycle_inputs(n, 0, mu[:, :4], seed=92)
    earth = onp.earth_rotation(s.ORIENT_LATITUDE)
    R = s.dense_process_noise_per_filter("orient", n) if per_filter else s.dense_process_noise("orient")
    m1, c1, s1 = oracle.orient_predict(mu, cov, R, acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, earth, DT)
    m2, c2, s2 = onp.orient_predict(mu, cov, R, acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, earth, DT)
    assert (s1 == 0).all() and (s2 == 0).all()
    assert max_abs(m1, m2) < 1e-12 and max_abs(c1, c2) < 1e-12
    _, c0, _ = onp.orient_predict(mu, cov, np.zeros((13, 13)), acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, earth, DT)
    assert max_abs(c1, c0) > 100 * TOL_F32


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_dense_noise_fixtures_have_the_claimed_structure(spe, model):
    s = spe.synth
    D = 12 if model == "pose" else 13
    low = np.tril_indices(D)
    Rs = s.dense_process_noise_per_filter(model, 64)
    assert np.array_equal(Rs[0], s.dense_process_noise(model))
    for R in Rs:
        assert np.array_equal(R, R.T) and np.linalg.eigvalsh(R).min() > 0
        v = R[low]
        assert (v != 0).all() and len(np.unique(v)) == v.size            # every lower-triangle entry nonzero and distinct
        for b in (0, 3):                                                  # the rotated blocks are anisotropic
            assert np.ptp(np.linalg.eigvalsh(R[b:b + 3, b:b + 3])) > 0.1 * R[b:b + 3, b:b + 3].trace() / 3
    assert all(not np.array_equal(Rs[i], Rs[j]) for i in range(4) for j in range(i))
    a = s.dense_acc_cov()
    assert np.array_equal(a, a.T) and (a != 0).all() and np.linalg.eigvalsh(a).min() > 0
    if model == "pose":                                                   # acceleration-branch form stays positive definite
        Ra = Rs.copy()
        Ra[:, 6:9, 6:9] = 2.0 * a
        assert np.linalg.eigvalsh(Ra).min() > 0


def _swap(R, i, j, k, l):
    """R with the symmetric pairs (i, j) and (k, l) exchanged."""
    R = R.copy()
    a, b = R[i, j], R[k, l]
    R[i, j] = R[j, i] = b
    R[k, l] = R[l, k] = a
    return R


def _swap_extremes(R, rows, cols):
    """R with the largest and the smallest entry strictly below the diagonal inside R[rows, cols] exchanged (with their mirror
    images)."""
    idx = [(i, j) for i in rows for j in cols if i > j]
    v = np.array([R[i, j] for i, j in idx])
    return _swap(R, *idx[int(v.argmax())], *idx[int(v.argmin())])


def _block_diagonal(R):
    out = np.zeros_like(R)
    for b in range(0, R.shape[0], 3):
        out[b:b + 3, b:b + 3] = R[b:b + 3, b:b + 3]
    if R.shape[0] % 3:
        out[-1, -1] = R[-1, -1]
    return out


def test_fixtures_tell_a_misaddressed_noise_entry_apart(spe, oracle):
    """A kernel that read two noise entries from each other's places, or read the blocks off the diagonal as zero, would give a
    predicted covariance 1e3 x the fp32 tolerance away from the oracle's: one swapped pair in a cross block, one inside a
    rotated block, for both models (the time step makes the scaled noise, dt R or dt^2 R, comparable to the raw one)."""
    s = spe.synth
    n = 16
    dt = 3.0
    mu, cov, _ = _pose_inputs(spe, n, 93)
    R = s.dense_process_noise("pose")
    _, c, _ = oracle.pose_predict(mu, cov, R, None, None, dt)
    for swapped in (_swap_extremes(R, range(6, 9), range(0, 3)),     # position <-> velocity cross block
                    _swap_extremes(R, range(0, 3), range(0, 3)),     # inside the rotated position block
                    _block_diagonal(R)):
        _, c2, _ = oracle.pose_predict(mu, cov, swapped, None, None, dt)
        assert max_abs(c, c2) >= 1e3 * TOL_F32
    mu, cov = s.orient_initial(n, seed=93)
    gyro, acc, _, _ = s.orient_cycle_inputs(n, 0, mu[:, :4], seed=93)
    earth = np.array([0.0, 0.0, 0.0])
    dt = 1.0
    R = s.dense_process_noise("orient")
    _, c, _ = oracle.orient_predict(mu, cov, R, acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, earth, dt)
    for swapped in (_swap_extremes(R, range(9, 12), range(3, 6)),    # velocity <-> acceleration bias cross block
                    _swap_extremes(R, range(3, 6), range(3, 6)),     # inside the rotated velocity block
                    _block_diagonal(R)):
        _, c2, _ = oracle.orient_predict(mu, cov, swapped, acc, gyro, s.ORIENT_TAU, s.ORIENT_TAU, earth, dt)
        assert max_abs(c, c2) >= 1e3 * TOL_F32


def _effective_noise(onp, R, q, dt, model):
    rot = onp.quat_to_matrix(q[None])[0]
    Re = R.copy()
    Re[0:3, 0:3] = rot @ R[0:3, 0:3] @ rot.T
    Re[3:6, 3:6] = rot @ R[3:6, 3:6] @ rot.T
    return (dt if model == "pose" else dt * dt) * Re


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_rotation_indefinite_noise_is_what_it_claims(spe, oracle, onp, model):
    """Raw R positive semidefinite, the noise the prediction adds at ROTATION_INDEFINITE_Q indefinite; the plain cycle's update
    fails its factorisation in the oracle (ST_ERR_CHOLESKY), while Sigma' computed the linear-Kalman way has a positive definite
    leading (RT + 3) x (RT + 3) block -- the part a short update factorisation reads -- so only the complete one catches it."""
    s = spe.synth
    q = s.ROTATION_INDEFINITE_Q
    R = s.rotation_indefinite_noise(model)
    dt = 0.1
    assert np.array_equal(R, R.T) and np.linalg.eigvalsh(R).min() >= 0
    assert np.linalg.eigvalsh(_effective_noise(onp, R, q, dt, model)).min() < -1e-4
    Q = 1e-2 * np.eye(3)[None]
    z = np.zeros((1, 3))
    if model == "pose":
        mu = np.zeros((1, 13)); mu[0, 3:7] = q
        cov = 1e-8 * np.eye(12)[None]
        m, c, s1 = oracle.pose_predict(mu, cov, R, None, None, dt)
        _, _, s2 = oracle.pose_update(m, c, spe.MEAS_POS3, z, Q)
        H = np.zeros((3, 12)); H[:, 0:3] = np.eye(3)
        lead = 6                                     # RT + 3, RT = 3
    else:
        mu = np.zeros((1, 14)); mu[0, 0:4] = q; mu[0, 13] = s.ORIENT_G
        cov = 1e-8 * np.eye(13)[None]
        acc = onp.quat_rotate(onp.quat_inverse(q[None]), np.array([[0.0, 0.0, s.ORIENT_G]]))
        m, c, s1 = oracle.orient_predict(mu, cov, R, acc, np.zeros((1, 3)), s.ORIENT_TAU, s.ORIENT_TAU,
                                         onp.earth_rotation(s.ORIENT_LATITUDE), dt)
        _, _, s2 = oracle.orient_update(m, c, z, Q)
        H = np.zeros((3, 13)); H[:, 3:6] = onp.quat_to_matrix(m[:, 0:4])[0].T    # d(q^-1 v) / dv at v = 0
        lead = 3                                     # RT + 3, RT = 0
    assert s1[0] == 0 and s2[0] == spe.ST_ERR_CHOLESKY
    P = c[0]
    assert np.linalg.eigvalsh(P).min() < 0
    S = H @ P @ H.T + Q[0]
    K = P @ H.T @ np.linalg.inv(S)
    P2 = P - K @ S @ K.T
    assert np.linalg.eigvalsh(P2).min() < -1e-4
    assert np.linalg.eigvalsh(P2[:lead, :lead]).min() > 0
    # orientations about the x axis keep the noise semidefinite: the same filter then updates cleanly
    qx = np.array([np.sin(0.35), 0.0, 0.0, np.cos(0.35)])
    assert np.linalg.eigvalsh(_effective_noise(onp, R, qx, dt, model)).min() > -1e-15
