"""NumPy float64 statement of the sensor-frame measurements of include/ukf_batch.h ("sensor-frame measurements"): the eight
h functions, and per model id the scored update of tests/update_reference.py on (POSE | ORIENT, VECT(m)):
oracle.ukf_numpy.ukf_update, what it does not return (z-bar, S, the innovation, the squared Mahalanobis distance, the
log-likelihood) and the status rules of the header.  A helper, not collected; tests/test_sensor_meas_reference.py pins it.

Conventions: R(q) x = on.quat_rotate(q, x); R(q)^T x = on.quat_rotate(on.quat_inverse(q), x) (what the reference library's
q.inverse() * x is); mount = r[3] then qs[4] (x, y, z, w); point = b[3]."""
import numpy as np

from oracle import ukf_numpy as on
from update_reference import nan_outputs, scored_update

LN_2PI = float(np.log(2.0 * np.pi))

POSE_POSITION, POSE_RANGE, POSE_POINT, POSE_VELOCITY, POSE_NAV_VELOCITY = 0, 1, 2, 3, 4
ORIENT_VELOCITY, ORIENT_NAV_VECTOR, ORIENT_SPECIFIC_FORCE = 5, 6, 7
POSE_IDS, ORIENT_IDS = (0, 1, 2, 3, 4), (5, 6, 7)
NAMES = {0: "POSE_POSITION", 1: "POSE_RANGE", 2: "POSE_POINT", 3: "POSE_VELOCITY", 4: "POSE_NAV_VELOCITY",
         5: "ORIENT_VELOCITY", 6: "ORIENT_NAV_VECTOR", 7: "ORIENT_SPECIFIC_FORCE"}
READS_LEVER, READS_ROTATION, READS_POINT = (0, 1, 2, 3, 5), (2, 3, 5, 6), (1, 2, 6)
IDENTITY_MOUNT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def meas_dim(mid):
    return 1 if mid == POSE_RANGE else 3


def ids_of(man):
    return POSE_IDS if man is on.POSE else ORIENT_IDS


def rot(q, x):
    return on.quat_rotate(q, x)


def rot_t(q, x):
    return on.quat_rotate(on.quat_inverse(q), x)


def h(mid, X, mount, point, gyro=None):
    """X [..., S]; mount [..., 7], point [..., 3], gyro [..., 3] broadcast against X's leading axes -> Z [..., m]"""
    r, qs, b = mount[..., 0:3], mount[..., 3:7], point
    if mid <= POSE_NAV_VELOCITY:
        p, q, v, w = X[..., 0:3], X[..., 3:7], X[..., 7:10], X[..., 10:13]
        if mid == POSE_POSITION:
            return p + rot(q, r)
        if mid == POSE_RANGE:
            u = (p - b) + rot(q, r)
            return np.sqrt(np.sum(u * u, axis=-1, keepdims=True))
        if mid == POSE_POINT:
            return rot_t(qs, rot_t(q, b - p) - r)
        if mid == POSE_VELOCITY:
            return rot_t(qs, v + np.cross(w, r))
        return rot(q, v)
    q, v, bg, ba, g = X[..., 0:4], X[..., 4:7], X[..., 7:10], X[..., 10:13], X[..., 13:14]
    if mid == ORIENT_VELOCITY:
        return rot_t(qs, rot_t(q, v) + np.cross(gyro - bg, r))
    if mid == ORIENT_NAV_VECTOR:
        return rot_t(qs, rot_t(q, b))
    return rot_t(q, np.concatenate([np.zeros(g.shape[:-1] + (2,)), g], axis=-1)) + ba


def used_inputs(mid):
    """(entries of z, mask of Q [3, 3], entries of mount [7], entries of point [3]) that model `mid` reads"""
    m = meas_dim(mid)
    qm = np.zeros((3, 3), bool)
    qm[:m, :m] = True
    mm = np.zeros(7, bool)
    mm[0:3] = mid in READS_LEVER
    mm[3:7] = mid in READS_ROTATION
    return np.arange(3) < m, qm, mm, np.full(3, mid in READS_POINT)


def update_sensor(man, mu, cov, models, z, Q, mount, point, gyro=None, gate_chi2=-1.0, initialised=None, tol=on.MEAN_TOL,
                  max_it=on.MEAN_MAX_IT):
    """mu [B, S], cov [B, D, D], models an int or [B], z [B, 3], Q [B, 3, 3] (or [3, 3]), mount [B, 7] (or [7]), point [B, 3]
    (or [3]), gyro [B, 3] (OrientationState) -> dict(mu, cov, z_pred [B, 3], S [B, 3, 3], innov [B, 3], maha [B], loglik [B],
    status [B]).  Filters are grouped by model id; every group is one scored update."""
    B = mu.shape[0]
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, 3, 3))
    mount = np.broadcast_to(np.asarray(mount, dtype=np.float64), (B, 7))
    point = np.broadcast_to(np.asarray(point, dtype=np.float64), (B, 3))
    gyro = np.zeros((B, 3)) if gyro is None else np.asarray(gyro, dtype=np.float64)
    init = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    o = nan_outputs(mu, cov, 3, 3)
    valid = np.isin(models, ids_of(man))
    o["status"][~init] = on.ST_UNINITIALISED
    o["status"][init & ~valid] = on.ST_INACTIVE
    for mid in np.unique(models[init & valid]):
        mid = int(mid)
        m = meas_dim(mid)
        idx = np.nonzero(init & valid & (models == mid))[0]
        o["innov"][idx, m:] = 0.0   # padding is 0 whatever becomes of the filter
        uz, uq, um, up = used_inputs(mid)
        fin = (np.isfinite(z[idx][:, uz]).all(axis=1) & np.isfinite(Q[idx][:, uq]).all(axis=1) &
               np.isfinite(mount[idx][:, um]).all(axis=1) & np.isfinite(point[idx][:, up]).all(axis=1))
        o["status"][idx[~fin]] = on.ST_ERR_NONFINITE_MEAS
        idx = idx[fin]
        if idx.size == 0:
            continue
        zz, QQ = z[idx][:, :m], Q[idx][:, :m, :m]
        # entries the model does not read never meet arithmetic
        mt = np.where(um, mount[idx], IDENTITY_MOUNT)[:, None, :]
        pt = np.where(up, point[idx], 0.0)[:, None, :]
        gy = gyro[idx][:, None, :]
        hh = lambda X: h(mid, X, mt, pt, gy)
        u = scored_update(man, on.VECT(m), mu[idx], cov[idx], zz, hh, QQ, tol, max_it, gate_chi2)
        o["mu"][idx[u.commit]], o["cov"][idx[u.commit]] = u.mu2[u.commit], u.cov2[u.commit]
        sc = idx[u.scored]
        o["z_pred"][sc] = 0.0
        o["z_pred"][sc, :m] = u.mz[u.scored]
        o["S"][sc] = 0.0
        o["S"][sc[:, None, None], np.arange(m)[None, :, None], np.arange(m)[None, None, :]] = u.S[u.scored]
        o["innov"][sc, :m] = u.innov[u.scored]
        o["maha"][sc] = u.d2[u.scored]
        o["loglik"][sc] = -0.5 * (u.d2[u.scored] + u.logdet[u.scored] + m * LN_2PI)
        o["status"][idx] = u.status
    return o
