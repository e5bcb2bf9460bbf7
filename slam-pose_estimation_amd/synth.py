"""Deterministic synthetic inputs for the UKF hot path.

Counter-based SplitMix64 so that any consumer (NumPy here, C++ elsewhere) draws the same
numbers from (seed, filter id, slot) without shared state.  All outputs are float64 AoS arrays in
the layout of include/ukf_batch.h (quaternions x, y, z, w).
"""
from __future__ import annotations

import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
SLOTS = 512  # stream index = filter id * SLOTS + slot

SEED_BASE = 0x5EED0000


def splitmix64(x):
    """SplitMix64 output function applied to the 64-bit counters x (vectorised)."""
    with np.errstate(over="ignore"):
        z = (np.asarray(x, dtype=np.uint64) + _GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return z


def uniform(seed: int, ids, slots, lo=0.0, hi=1.0):
    """U(lo, hi) from the top 53 bits; result shape = broadcast(ids[:, None], slots[None, :])."""
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1, 1)
    slots = np.asarray(slots, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over="ignore"):
        ctr = (ids * np.uint64(SLOTS) + slots) * _GOLDEN + splitmix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF))
    u = (splitmix64(ctr) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return lo + (hi - lo) * u


def _quat_exp(a):
    """MTK SO3::exp(a) with scale 1 (plain sin/cos form; generator only, not part of parity)."""
    n = np.linalg.norm(a, axis=-1, keepdims=True)
    half = 0.5 * n
    s = np.where(n > 1e-12, np.sin(half) / np.where(n > 1e-12, n, 1.0), 0.5)
    return np.concatenate([a * s, np.cos(half)], axis=-1)


def _spd(seed, ids, dof, diag_std, slot0=16):
    """Sigma0 = D^1/2 (I + 0.1 G G^T / dof) D^1/2 with G ~ U(-1,1)^(dof x dof)."""
    n = len(ids)
    G = uniform(seed, ids, np.arange(slot0, slot0 + dof * dof), -1.0, 1.0).reshape(n, dof, dof)
    A = np.eye(dof)[None] + 0.1 * (G @ np.swapaxes(G, 1, 2)) / float(dof)
    d = np.asarray(diag_std, dtype=np.float64)
    C = d[None, :, None] * A * d[None, None, :]
    return 0.5 * (C + np.swapaxes(C, 1, 2))  # exactly symmetric


# ------------------------------------------------------------------------------- Pose
POSE_DIAG_STD = np.array([0.1] * 3 + [0.05] * 3 + [0.1] * 3 + [0.02] * 3)


def pose_default_process_noise():
    """PoseUKF ctor defaults (PoseUKF.cpp:103-107 of the reference)."""
    return np.diag([0.01] * 3 + [0.001] * 3 + [0.00001] * 3 + [0.00001] * 3)


def pose_initial(n: int, seed: int = SEED_BASE + 2, first: int = 0):
    """mu [n,13], cov [n,12,12]."""
    ids = np.arange(first, first + n)
    p = uniform(seed, ids, [0, 1, 2], -10.0, 10.0)
    q = _quat_exp(uniform(seed, ids, [3, 4, 5], -1.0, 1.0))
    v = uniform(seed, ids, [6, 7, 8], -1.0, 1.0)
    w = uniform(seed, ids, [9, 10, 11], -0.2, 0.2)
    mu = np.concatenate([p, q, v, w], axis=-1)
    cov = _spd(seed, ids, 12, POSE_DIAG_STD)
    return mu, cov


def pose_cycle_inputs(n: int, cycle: int, mu_pos=None, seed: int = SEED_BASE + 2, first: int = 0, random_q=False):
    """Per-cycle inputs: acc [n,3], z [n,3] (= position + noise when mu_pos is given, else U(-10,10)+noise),
    Q [n,3,3] (0.05^2 I, or random SPD when random_q)."""
    ids = np.arange(first, first + n)
    s = seed + 0x10000 * (cycle + 1)
    acc = uniform(s, ids, [0, 1, 2], -0.5, 0.5)
    noise = uniform(s, ids, [3, 4, 5], -0.05, 0.05)
    base = mu_pos if mu_pos is not None else uniform(seed, ids, [0, 1, 2], -10.0, 10.0)
    z = base + noise
    if random_q:
        G = uniform(s, ids, np.arange(6, 15), -1.0, 1.0).reshape(n, 3, 3)
        Q = 0.05 ** 2 * (np.eye(3)[None] + 0.3 * (G @ np.swapaxes(G, 1, 2)) / 3.0)
        Q = 0.5 * (Q + np.swapaxes(Q, 1, 2))
    else:
        Q = np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)).copy()
    return acc, z, Q


def pose_mixed_models(n: int, cycle: int, seed: int = SEED_BASE + 5, first: int = 0, inactive_frac=0.25):
    """Config 5: per-filter measurement model id uniform over the 9 Pose models, -1 for inactive."""
    ids = np.arange(first, first + n)
    s = seed + 0x10000 * (cycle + 1)
    m = np.floor(uniform(s, ids, [15], 0.0, 9.0)).astype(np.int32).reshape(-1)
    m = np.clip(m, 0, 8)
    off = uniform(s, ids, [16]).reshape(-1) < inactive_frac
    return np.where(off, -1, m).astype(np.int32)


def pose_measurement_for_model(mu, models, noise):
    """z [n,3] consistent with each filter's model id (first m entries used)."""
    n = mu.shape[0]
    z = np.zeros((n, 3))
    sel = {0: [0, 1, 2], 1: [0, 1], 2: [2], 4: [7, 8, 9], 5: [7, 8], 6: [9], 7: [7, 12], 8: [10, 11, 12]}
    for mid, idx in sel.items():
        i = np.nonzero(models == mid)[0]
        z[np.ix_(i, range(len(idx)))] = mu[np.ix_(i, idx)] + noise[np.ix_(i, range(len(idx)))]
    i = np.nonzero(models == 3)[0]
    if len(i):
        # axis-angle of the current orientation plus noise (log map of a unit quaternion)
        q = mu[i, 3:7]
        nv = np.linalg.norm(q[:, :3], axis=-1, keepdims=True)
        ang = 2.0 * np.arctan2(nv, q[:, 3:4])
        axis = q[:, :3] / np.where(nv > 1e-12, nv, 1.0)
        z[i] = axis * ang + noise[i]
    return z


# ------------------------------------------------------------------------------- Orient
ORIENT_DIAG_STD = np.array([0.05] * 3 + [0.1] * 3 + [0.001] * 3 + [0.01] * 3 + [0.01])
ORIENT_LATITUDE = 0.92698121
ORIENT_TAU = 3600.0
ORIENT_G = 9.81


def orient_process_noise():
    """SURVEY.md section 8(d) config 4 (the reference default is zero)."""
    return np.diag([1e-6] * 3 + [1e-4] * 3 + [1e-10] * 3 + [1e-8] * 3 + [1e-12])


def orient_initial(n: int, seed: int = SEED_BASE + 4, first: int = 0):
    """mu [n,14] = q, v, bias_gyro, bias_acc, gravity; cov [n,13,13]."""
    ids = np.arange(first, first + n)
    q = _quat_exp(uniform(seed, ids, [0, 1, 2], -1.0, 1.0))
    v = uniform(seed, ids, [3, 4, 5], -1.0, 1.0)
    bg = uniform(seed, ids, [6, 7, 8], -1e-3, 1e-3)
    ba = uniform(seed, ids, [9, 10, 11], -1e-2, 1e-2)
    g = np.full((n, 1), ORIENT_G)
    mu = np.concatenate([q, v, bg, ba, g], axis=-1)
    cov = _spd(seed, ids, 13, ORIENT_DIAG_STD, slot0=16)
    return mu, cov


def orient_cycle_inputs(n: int, cycle: int, mu_q=None, seed: int = SEED_BASE + 4, first: int = 0):
    """gyro [n,3], acc [n,3] = q^-1 (0,0,g) + U(-0.1,0.1)^3, z [n,3], Q [n,3,3]."""
    ids = np.arange(first, first + n)
    s = seed + 0x10000 * (cycle + 1)
    gyro = uniform(s, ids, [0, 1, 2], -0.2, 0.2)
    if mu_q is None:
        mu_q = _quat_exp(uniform(seed, ids, [0, 1, 2], -1.0, 1.0))
    # rotate (0,0,g) by q^-1
    qv = -mu_q[:, :3]
    w = mu_q[:, 3:4]
    gvec = np.broadcast_to(np.array([0.0, 0.0, ORIENT_G]), (n, 3))
    uv = 2.0 * np.cross(qv, gvec)
    grav_body = gvec + w * uv + np.cross(qv, uv)
    acc = grav_body + uniform(s, ids, [3, 4, 5], -0.1, 0.1)
    z = uniform(s, ids, [6, 7, 8], -0.05, 0.05)
    Q = np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)).copy()
    return gyro, acc, z, Q


# ------------------------------------------------------------------------------- dense process noise (tests)
# Process noise whose every lower-triangle entry is nonzero and distinct: a kernel that reads one entry of the noise from the
# wrong place (a swapped pair, a cross block read as zero) changes the predicted covariance.  Standard deviations per state
# dimension: the noise moves the predicted covariance by ~1e-3 .. 1e-2 at dt = 0.01 .. 0.05 (Pose, constant-velocity branch:
# dt R; OrientationState: dt^2 R), far above the fp32 tolerance, while the orientation blocks stay small enough for ordinary
# sigma-point spreads.  The Pose velocity block stays below 2 dense_acc_cov(), so the acceleration branch's noise (velocity
# block replaced by 2 acc.cov, PoseUKF.cpp:190-191) stays positive definite as well.
DENSE_NOISE_STD = {
    "pose": np.array([1.0] * 3 + [0.03] * 3 + [0.3] * 3 + [0.3] * 3),
    "orient": np.array([1.0] * 3 + [3.0] * 3 + [0.3] * 3 + [3.0] * 3 + [3.0]),
}
ROTATION_INDEFINITE_Q = np.array([0.5, 0.5, 0.5, 0.5])   # (x, y, z, w): a rotation by 120 degrees that moves every axis


def _dense_spd(seed, ids, std):
    """S^1/2 C S^1/2: C the correlation matrix of I / 8 + G G^T / dof, G ~ U(-1, 1)^(dof x dof) (correlations of both signs, no
    entry zero), S = std^2 times U(1, 2) per entry of the diagonal (no two variances equal)."""
    n, dof = len(ids), len(std)
    G = uniform(seed, ids, np.arange(dof * dof), -1.0, 1.0).reshape(n, dof, dof)
    A = 0.125 * np.eye(dof)[None] + (G @ np.swapaxes(G, 1, 2)) / float(dof)
    d = 1.0 / np.sqrt(np.einsum("nii->ni", A))
    sd = std[None, :] * np.sqrt(uniform(seed, ids, np.arange(dof * dof, dof * dof + dof), 1.0, 2.0))
    C = (d[:, :, None] * A * d[:, None, :]) * (sd[:, :, None] * sd[:, None, :])
    C = 0.5 * (C + np.swapaxes(C, 1, 2))
    # The prediction rotates the diagonal blocks [0:3] and [3:6] and keeps everything else (not a congruence): scale the entries
    # coupling the three groups [0:3], [3:6], [6:] so that the noise stays positive definite for ANY rotation.  With the groups'
    # smallest eigenvalues l (invariant under the rotation) and X the coupling entries, ||diag(l)^-1/2 X diag(l)^-1/2|| <= 1/2.
    grp = np.minimum(np.arange(dof) // 3, 2)
    cross = grp[:, None] != grp[None, :]
    lam = np.empty((n, dof))
    for g in range(3):
        lam[:, grp == g] = np.linalg.eigvalsh(C[:, grp == g][:, :, grp == g]).min(axis=1)[:, None]
    X = np.where(cross[None], C, 0.0)
    K = X / np.sqrt(lam[:, :, None] * lam[:, None, :])
    t = np.minimum(1.0, 0.5 / np.linalg.norm(K, ord=2, axis=(1, 2)))
    return np.where(cross[None], C * t[:, None, None], C)


def dense_process_noise_per_filter(model: str, n: int, seed: int = SEED_BASE + 7):
    """[n, D, D]: a different dense positive definite process noise per filter (model "pose" or "orient")."""
    return _dense_spd(seed, np.arange(n), DENSE_NOISE_STD[model])


def dense_process_noise(model: str, seed: int = SEED_BASE + 7):
    """[D, D]: one dense positive definite process noise (model "pose" or "orient"); = filter 0 of the per-filter stack."""
    return dense_process_noise_per_filter(model, 1, seed)[0]


def dense_acc_cov(seed: int = SEED_BASE + 8):
    """A full SPD 3x3 acceleration covariance, eigenvalues >= 0.3 (see DENSE_NOISE_STD)."""
    G = uniform(seed, [0], np.arange(9), -1.0, 1.0).reshape(3, 3)
    A = 0.3 * np.eye(3) + 0.05 * (G @ G.T)
    return 0.5 * (A + A.T)


def rotation_indefinite_noise(model: str):
    """A positive semidefinite process noise that the prediction makes INDEFINITE at the orientation ROTATION_INDEFINITE_Q: the
    prediction rotates the diagonal blocks [0:3] and [3:6] but leaves their cross blocks raw (PoseUKF.cpp:184-185,
    OrientationUKF.cpp:84-85), which is not a congruence.  An anisotropic rotated block (variance along x only) is coupled almost
    perfectly to a block that is not rotated: Pose position x <-> velocity x, OrientationState velocity x <-> acceleration bias x.
    Orientations that keep the x axis (rotations about x) keep the noise semidefinite."""
    if model == "pose":
        R = np.diag(np.r_[1e-2 * np.array([1.0, 1e-6, 1e-6]), [1e-3] * 3, [1e-2] * 3, [1e-5] * 3])
        R[0, 6] = R[6, 0] = 0.99e-2
    else:
        R = np.diag(np.r_[[1e-3] * 3, [1.0, 1e-6, 1e-6], [1e-4] * 3, [1.0] * 3, [1e-4]])
        R[3, 9] = R[9, 3] = 0.99
    return R
