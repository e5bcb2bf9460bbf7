"""NumPy float64 statement of the user-defined measurement models of include/ukf_batch.h ("user-defined measurement models"):
the sigma-point export in its filter-major layout, and the scored update of tests/update_reference.py on (POSE | ORIENT,
VECT(m)) with h = the caller's samples: oracle.ukf_numpy.ukf_update, what it does not return (z-bar, S, the innovation, the
squared Mahalanobis distance, the log-likelihood) and the status rules of the header.  A helper, not collected;
tests/test_sampled_reference.py pins it."""
import numpy as np

from oracle import ukf_numpy as on
from update_reference import nan_outputs, scored_update

LN_2PI = float(np.log(2.0 * np.pi))
MAX_M = 6


def sigma_points(man, mu, cov, initialised=None):
    """-> (X [B, 2 D + 1, S], delta [B, 2 D + 1, D], status [B]): point 0 = mu, 1 + 2 j = mu (+) L col j, 2 + 2 j =
    mu (+) (-L col j); rows of NaN and UNINITIALISED / ERR_CHOLESKY for a filter that has no points"""
    B, D = mu.shape[0], man.D
    init = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    L, ok = on.cholesky_lower(np.where(init[:, None, None], cov, np.eye(D)))
    good = init & ok
    safe_cov = np.where(good[:, None, None], cov, np.eye(D))
    X, _ = on.sigma_points(man, mu, safe_cov)
    L, _ = on.cholesky_lower(safe_cov)
    delta = np.zeros((B, 2 * D + 1, D))
    for j in range(D):
        delta[:, 1 + 2 * j] = L[:, :, j]
        delta[:, 2 + 2 * j] = -L[:, :, j]
    X[:, 0] = mu   # bit for bit
    X[~good], delta[~good] = np.nan, np.nan
    status = np.where(~init, on.ST_UNINITIALISED, np.where(~ok, on.ST_ERR_CHOLESKY, 0)).astype(np.uint32)
    return X, delta, status


def update_sampled(man, mu, cov, Z, z, Q, active=None, gate_chi2=-1.0, initialised=None, tol=on.MEAN_TOL, max_it=on.MEAN_MAX_IT):
    """mu [B, S], cov [B, D, D], Z [B, 2 D + 1, m], z [B, m], Q [B, m, m] (or [m, m]), active [B] or None -> dict(mu, cov,
    z_pred [B, m], S [B, m, m], innov [B, m], maha [B], loglik [B], status [B]): one scored update over the filters that take
    part"""
    B, m = mu.shape[0], Z.shape[2]
    assert 1 <= m <= MAX_M and Z.shape == (B, 2 * man.D + 1, m) and z.shape == (B, m)
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, m, m))
    init = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    act = np.ones(B, bool) if active is None else np.asarray(active) != 0
    o = nan_outputs(mu, cov, m, m)
    o["status"][~init] = on.ST_UNINITIALISED
    o["status"][init & ~act] = on.ST_INACTIVE
    lower = np.tril(np.ones((m, m), bool))
    fin = np.isfinite(z).all(axis=1) & np.isfinite(Q[:, lower]).all(axis=1) & np.isfinite(Z).all(axis=(1, 2))
    o["status"][init & act & ~fin] = on.ST_ERR_NONFINITE_MEAS
    idx = np.nonzero(init & act & fin)[0]
    if idx.size == 0:
        return o
    zz, ZZ = z[idx], Z[idx]
    QQ = np.where(lower, Q[idx], np.swapaxes(Q[idx], 1, 2))   # the lower triangle is what is read
    u = scored_update(man, on.VECT(m), mu[idx], cov[idx], zz, lambda X: ZZ, QQ, tol, max_it, gate_chi2)
    o["mu"][idx[u.commit]], o["cov"][idx[u.commit]] = u.mu2[u.commit], u.cov2[u.commit]
    sc = idx[u.scored]
    o["z_pred"][sc], o["S"][sc], o["innov"][sc] = u.mz[u.scored], u.S[u.scored], u.innov[u.scored]
    o["maha"][sc] = u.d2[u.scored]
    o["loglik"][sc] = -0.5 * (u.d2[u.scored] + u.logdet[u.scored] + m * LN_2PI)
    o["status"][idx] = u.status
    return o


# ------------------------------------------------------------------------------------------- a family of user-defined models
# The h functions the tests evaluate on exported sigma points: written once, over slices and arithmetic only, so that NumPy (the
# CPU tests) and torch on the device (the GPU tests: "Z = h(X) as a torch expression") run the same statements.  b [.., 3] is a
# nav-frame point (OrientationState: a nav-frame vector), r [.., 3] a lever arm; both broadcast against X's leading axes.
USER_DIMS = (1, 2, 3, 4, 6)


def _cat(parts):
    lib = np if isinstance(parts[0], np.ndarray) else __import__("torch")
    return lib.concatenate(parts, axis=-1) if lib is np else lib.cat(parts, dim=-1)


def _cross(a, b):
    return _cat([a[..., 1:2] * b[..., 2:3] - a[..., 2:3] * b[..., 1:2], a[..., 2:3] * b[..., 0:1] - a[..., 0:1] * b[..., 2:3],
                 a[..., 0:1] * b[..., 1:2] - a[..., 1:2] * b[..., 0:1]])


def _norm(u):
    return (u[..., 0:1] * u[..., 0:1] + u[..., 1:2] * u[..., 1:2] + u[..., 2:3] * u[..., 2:3]) ** 0.5


def rot(q, v):
    """R(q) v as oracle.ukf_numpy.quat_rotate"""
    qv = q[..., 0:3]
    uv = _cross(qv, v + 0.0 * qv)
    uv = uv + uv
    return v + q[..., 3:4] * uv + _cross(qv, uv)


def rot_t(q, v):
    """R(q)^T v: the rotation by q^-1 = conj(q) / |q|^2"""
    n2 = q[..., 0:1] * q[..., 0:1] + q[..., 1:2] * q[..., 1:2] + q[..., 2:3] * q[..., 2:3] + q[..., 3:4] * q[..., 3:4]
    return rot(_cat([-q[..., 0:3] / n2, q[..., 3:4] / n2]), v)


def user_h(model, m, X, b, r):
    """Pose: 1 range to b from the lever arm's end; 2 range and range rate; 3 b seen from the body; 4 its unit bearing and the
    range; 6 p + R(q) r stacked on R(q) v.  OrientationState: 1 |v - b|; 2 the horizontal body velocity; 3 R(q)^T b; 4 the
    unit bearing of R(q)^T (b - v) and its length; 6 R(q)^T b stacked on R(q)^T (0, 0, g) + b_a."""
    if model == "pose":
        p, q, v = X[..., 0:3], X[..., 3:7], X[..., 7:10]
        if m == 1:
            return _norm((p - b) + rot(q, r))
        if m == 2:
            d = p - b
            rho = _norm(d)
            w = rot(q, v)
            return _cat([rho, (d[..., 0:1] * w[..., 0:1] + d[..., 1:2] * w[..., 1:2] + d[..., 2:3] * w[..., 2:3]) / rho])
        if m == 3:
            return rot_t(q, b - p)
        if m == 4:
            u = rot_t(q, b - p)
            rho = _norm(u)
            return _cat([u / rho, rho])
        return _cat([p + rot(q, r), rot(q, v)])
    q, v, ba, g = X[..., 0:4], X[..., 4:7], X[..., 10:13], X[..., 13:14]
    if m == 1:
        return _norm(v - b)
    if m == 2:
        return rot_t(q, v)[..., 0:2]
    if m == 3:
        return rot_t(q, b + 0.0 * v)
    if m == 4:
        u = rot_t(q, b - v)
        rho = _norm(u)
        return _cat([u / rho, rho])
    return _cat([rot_t(q, b + 0.0 * v), rot_t(q, _cat([0.0 * g, 0.0 * g, g])) + ba])


def make_inputs(model, mu, dtype, seed=11):
    """-> (b [n, 3], r [n, 3], {m: noise [n, m]}, {m: Q [n, m, m]}) as the engine stores them: points 15 ... 80 m from the filter
    (OrientationState: from the origin), lever arms U(-1, 1)^3, z = h(mu) + noise with noise = 0.05 N(0, 1), Q = 0.05^2 (I + G G^T /
    (4 m)) with G ~ N(0, 1)^(m x m): dense, so that the row-major m x m indexing is exercised"""
    n = mu.shape[0]
    rng = np.random.default_rng(seed)
    st = lambda x: np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)   # noqa: E731
    d = rng.standard_normal((n, 3))
    away = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(15.0, 80.0, (n, 1))
    b = st((mu[:, 0:3] + away) if model == "pose" else away)
    r = st(rng.uniform(-1.0, 1.0, (n, 3)))
    noise, Q = {}, {}
    for m in USER_DIMS:
        noise[m] = 0.05 * rng.standard_normal((n, m))
        G = rng.standard_normal((n, m, m))
        Q[m] = st(0.05 ** 2 * (np.eye(m) + G @ np.swapaxes(G, 1, 2) / (4.0 * m)))
        Q[m] = np.where(np.tril(np.ones((m, m), bool)), Q[m], np.swapaxes(Q[m], 1, 2))   # symmetric as stored
    return b, r, noise, Q
