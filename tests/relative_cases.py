"""Inputs of the relative-measurement tests (tests/test_relative_reference.py on the CPU, tests/test_gpu_relative.py on the
device): the linear (p, v) system with its textbook cloned Kalman filter, the hot Pose history by the NumPy oracle, the increments
drawn near the truth, and the recorder that fills a history ring with history_push_dev during real cycles.  A helper, not
collected.  The linear system and the hot history are those of tests/test_delayed_reference.py and tests/test_gpu_delayed.py
(no test imports a test: the few statements are repeated here, Pose only)."""
import numpy as np

from oracle import ukf_numpy as on
import delayed_reference as dr
import relative_reference as rr
import smoother_reference as sr

ACC_COV = 0.01 * np.eye(3)
PV = [0, 1, 2, 6, 7, 8]          # tangent indices of (p, v) in PoseWithVelocity
PVS = [0, 1, 2, 7, 8, 9]         # ... and the stored ones

# ------------------------------------------------------------------------------------------------ the linear (p, v) system
ROT_VAR = 1e-12
Q6 = np.zeros((6, 6)); Q6[:3, :3] = 0.01 * np.eye(3); Q6[3:, 3:] = 2.0 * ACC_COV
R_POS, R_REL = 0.05 ** 2 * np.eye(3), 0.03 ** 2 * np.eye(3)
H_POS = np.eye(6)[:3]


def kf_update(x, P, z, H, R):
    S = H @ P @ H.T + R
    K = P @ H.T @ np.linalg.inv(S)
    return x + np.einsum("bij,bj->bi", K, z - x @ H.T), P - K @ S @ np.swapaxes(K, -1, -2)


def linear_filter(steps, B, clone_at=None, z_rel=None, seed=5):
    """The textbook Kalman filter of Pose's (p, v) at identity orientation, zero angular velocity, the acceleration branch
    (p' = p + dt v + dt^2 a, v' = v + dt a, the raw noise) with a position fix at every step -> (x [steps, B, 6],
    P [steps, B, 6, 6], dt, acc).  clone_at = s: from step s on the filter carries a clone of x_s explicitly (12 states), and
    at the last step the relative position z_rel = p_n - p_s + noise (R_REL) is processed; the returned records are the first
    six states."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-5, 5, (B, 3)), rng.uniform(-1, 1, (B, 3))], axis=-1)
    G = rng.uniform(-1, 1, (B, 6, 6))
    P = 0.01 * (np.eye(6) + G @ np.swapaxes(G, -1, -2) / 6.0)
    dt = 0.02 + 0.03 * rng.uniform(0, 1, steps - 1)
    acc = rng.uniform(-0.5, 0.5, (steps, B, 3))
    zs = rng.uniform(-5, 5, (steps, B, 3))
    nx = 6
    H = H_POS
    xs, Ps = [], []
    for c in range(steps):
        if c > 0:
            F = np.eye(nx); F[:3, 3:6] = dt[c - 1] * np.eye(3)
            u = np.zeros((B, nx)); u[:, :3] = dt[c - 1] ** 2 * acc[c - 1]; u[:, 3:6] = dt[c - 1] * acc[c - 1]
            Qa = np.zeros((nx, nx)); Qa[:6, :6] = Q6
            x = x @ F.T + u
            P = F @ P @ F.T + Qa
            x, P = kf_update(x, P, zs[c], H, R_POS)
        if clone_at == c:
            x = np.concatenate([x, x], axis=-1)
            P = np.block([[P, P], [P, P]])
            nx = 12
            H = np.concatenate([H_POS, np.zeros((3, 6))], axis=1)
        if clone_at is not None and c == steps - 1:
            Hr = np.zeros((3, 12)); Hr[:, 0:3] = np.eye(3); Hr[:, 6:9] = -np.eye(3)
            x, P = kf_update(x, P, z_rel, Hr, R_REL)
        xs.append(x[:, :6]); Ps.append(P[:, :6, :6])
    return np.array(xs), np.array(Ps), dt, acc


def embed(x, P):
    """(p, v) records -> PoseWithVelocity records: identity orientation, zero angular velocity, ROT_VAR on their diagonals"""
    steps, B = x.shape[:2]
    mu = np.zeros((steps, B, 13)); mu[..., 6] = 1.0
    mu[..., PVS] = x
    cov = np.zeros((steps, B, 12, 12))
    cov[np.ix_(range(steps), range(B), PV, PV)] = P
    for k in (3, 4, 5, 9, 10, 11):
        cov[..., k, k] = ROT_VAR
    return mu, cov


def linear_params():
    return sr.Params("pose", np.diag([0.01] * 3 + [ROT_VAR] * 3 + [0.0] * 3 + [ROT_VAR] * 3), acc_cov=ACC_COV)


# ------------------------------------------------------------------------------------------------ the hot Pose history
def cpu_history(spe, n, steps):
    """the recording of tests/test_gpu_relative.py with the NumPy oracle as the filter -> (params, mu [steps, n, S],
    cov [steps, n, D, D], dt, in_a [steps, n, 3])"""
    sy = spe.synth
    p = dr.hot_params(sy, "pose", ACC_COV)
    dt = np.array([dr.HOT_DT * (1.0 + 0.1 * c) for c in range(steps - 1)])
    mu, cov = dr.hot_initial(sy, "pose", n)
    mus, covs, ia = [], [], []
    a = None
    for c in range(steps):
        a_, _, mid, z, Q = dr.hot_cycle_inputs(sy, "pose", n, c, mu)
        if c > 0:
            mu, cov, s1 = on.pose_predict(mu, cov, p.R, a, ACC_COV, dt[c - 1])
            mu, cov, s2 = on.pose_update(mu, cov, mid, z, Q)
            assert not s1.any() and not s2.any()
        a = a_
        mus.append(mu); covs.append(cov); ia.append(a)
    return p, np.array(mus), np.array(covs), dt, np.array(ia)


# one dense 6 x 6 sample covariance in the tangent order (dp, dtheta): 3 cm and 0.02 rad, correlated across the two parts
_QA = np.array([[1.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.2, 1.0, 0.0, 0.0, 0.0, 0.0], [-0.1, 0.3, 1.0, 0.0, 0.0, 0.0],
                [0.2, -0.1, 0.1, 1.0, 0.0, 0.0], [0.0, 0.2, -0.2, 0.3, 1.0, 0.0], [0.1, 0.0, 0.2, -0.2, 0.1, 1.0]])
_QS = np.diag([0.03] * 3 + [0.02] * 3)
Q_REL = _QS @ _QA @ _QA.T @ _QS


def increments(spe, n, mu_n, mu_s, seed_offset=31):
    """-> (models [n] cycling through the three, z [n, 7], Q [6, 6]): the increment between the states mu_s and mu_n, every
    component 0.8 ... 1.6 sample sigmas off so that every sample matters.  The part a model does not read is NaN."""
    sy = spe.synth
    noise = sy.uniform(sy.SEED_BASE + seed_offset, np.arange(n), np.arange(6), -1.0, 1.0)
    noise = np.sign(noise) * (0.8 + 0.8 * np.abs(noise)) * np.sqrt(np.diag(Q_REL))
    z = rr.RZ.boxplus(rr.h_pair(mu_n, mu_s), noise)
    models = (np.arange(n) % 3).astype(np.int32)
    z[models == rr.POSITION, 3:] = np.nan
    z[models == rr.ROTATION, :3] = np.nan
    return models, z, Q_REL.copy()


# ------------------------------------------------------------------------------------------------ the device recorder
class Recording:
    """an engine at the window's last step, its history rings on the device, the inputs of every step"""


def record(spe, n, prec, wide, steps, slots, first, skip_init=(), **kw):
    """`steps` steps of real Pose cycles on the hot inputs, the filtered state of every step pushed into a ring of `slots`
    starting at slot `first` (tests/test_gpu_delayed.record, Pose only)"""
    import torch
    from engine_support import dev, new_engine, tdt
    sy = spe.synth
    e = new_engine(spe, "pose", n, prec, wide, **kw)
    mu0, cov0 = dr.hot_initial(sy, "pose", n)
    live = np.ones(n, bool)
    live[list(skip_init)] = False
    if skip_init:
        for i in np.nonzero(live)[0]:
            e.initialize(mu0[i:i + 1], cov0[i:i + 1], first=int(i))
    else:
        e.initialize(mu0, cov0)
    r = Recording()
    r.e, r.n, r.steps, r.slots, r.first, r.live = e, n, steps, slots, first, live
    r.mu_hist = torch.zeros((slots, n, e.S), dtype=tdt(e), device="cuda")
    r.cov_hist = torch.zeros((slots, n, e.PK), dtype=tdt(e), device="cuda")
    r.in_a = torch.zeros((slots, n, 3), dtype=tdt(e), device="cuda")
    r.dt = np.array([dr.HOT_DT * (1.0 + 0.1 * (c % 7)) for c in range(steps - 1)])
    for c in range(steps):
        slot = (first + c) % slots
        mu_now = np.where(live[:, None], e.state(with_cov=False)[0], mu0)
        a, _, mid, z, Q = dr.hot_cycle_inputs(sy, "pose", n, c, mu_now)
        if c > 0:
            e.cycle(float(r.dt[c - 1]), int(mid), z, Q)
        e.history_push_dev(slots, slot, r.mu_hist, r.cov_hist)
        e.set_acceleration(a, ACC_COV)
        r.in_a[slot] = dev(e, a)
    return r


def params(r):
    """smoother_reference.Params of a recording's engine, the noise as the engine stores it"""
    e = r.e
    R = np.asarray(e.process_noise(), dtype=e.dtype).astype(np.float64)
    cfg = e.config()
    return sr.Params("pose", R, acc_cov=np.asarray(2.0 * ACC_COV, dtype=e.dtype).astype(np.float64) / 2.0,
                     min_dt=cfg.min_time_delta, max_dt=cfg.max_time_delta)
