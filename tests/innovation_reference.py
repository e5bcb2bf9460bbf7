"""NumPy statement of the innovation statistics (ukfb_innovation_dev, include/ukf_batch.h) and the clutter the tests score:
ukfom's update up to S through the oracle's sigma points, then nu, d^2 and the log-likelihood of every candidate.  `onp` is
oracle.ukf_numpy, `spe` the package (for synth)."""
import numpy as np

K = 4
LN2PI = float(np.log(2.0 * np.pi))
POSE_MODELS = list(range(9))


def reference(onp, kind, mid, mu, cov, Q):
    """(m, manz, mz [n, S_z], S [n, m, m], ok, conv) of ukfom's update up to S"""
    if kind == "orient":
        man, manz, m = onp.ORIENT, onp.VECT(3), 3
        h = lambda X: onp.quat_rotate(onp.quat_inverse(X[..., 0:4]), X[..., 4:7])
    elif mid == 3:
        man, manz, m = onp.POSE, onp.SO3, 3
        h = lambda X: X[..., 3:7]
    else:
        idx = onp._POSE_SELECT[mid]
        man, manz, m = onp.POSE, onp.VECT(len(idx)), len(idx)
        h = lambda X: X[..., idx]
    X, ok = onp.sigma_points(man, mu, cov)
    Z = h(X)
    mz, conv = onp.mean_sigma_points(manz, Z)
    S = onp.cov_sigma_points(manz, mz, Z) + Q[:, :m, :m]
    return m, manz, mz, S, ok, conv


def reference_scores(onp, mid_is_so3, m, manz, mz, S, z):
    """nu [K, n, m], d2 [K, n], loglik [K, n] of candidates z [K, n, 3]"""
    Si = np.linalg.inv(S)
    logdet = np.log(np.linalg.det(S))
    nu, d2 = [], []
    for k in range(z.shape[0]):
        zk = onp.so3_exp(z[k], 1.0) if mid_is_so3 else z[k][:, :m]
        v = manz.boxminus(zk, mz)
        nu.append(v)
        d2.append(np.einsum("bi,bij,bj->b", v, Si, v))
    nu, d2 = np.array(nu), np.array(d2)
    return nu, d2, -0.5 * (d2 + logdet[None] + m * LN2PI)


def h_of_mean(onp, spe, kind, mid, mu, n):
    if kind == "orient":
        return onp.quat_rotate(onp.quat_inverse(mu[:, 0:4]), mu[:, 4:7])
    return spe.synth.pose_measurement_for_model(mu, np.full(n, mid, dtype=np.int32), np.zeros((n, 3)))


def clutter(onp, spe, kind, mid, mu, seed=0):
    """z_k = h(mu) + s (0.3 + k) U(-1, 1)^m, k = 0 ... 3; s = 0.15 (vector models), 0.08 rad (SO(3) axis-angle)"""
    n = mu.shape[0]
    s = 0.08 if (kind == "pose" and mid == 3) else 0.15
    hm = h_of_mean(onp, spe, kind, mid, mu, n)
    u = spe.synth.uniform(spe.synth.SEED_BASE + 21 + seed, np.arange(n), np.arange(3 * K), -1.0, 1.0).reshape(n, K, 3)
    return np.array([hm + s * (0.3 + k) * u[:, k] for k in range(K)])
