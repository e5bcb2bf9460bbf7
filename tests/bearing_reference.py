"""NumPy float64 statement of the bearing measurements of include/ukf_batch.h ("bearing measurements"): the three direction
models, the sphere S^2 as a measurement manifold for the oracle's own pieces (on.sigma_points, on.mean_sigma_points,
on.cov_sigma_points, on.ukf_update, which are duck-typed on the manifold), and on it the scored update of
tests/update_reference.py with the status rules of the header.  A helper, not collected; tests/test_bearing_reference.py pins
it.

The update is stated in the 2 x 2 BASIS FORM: S2 carries an explicit orthonormal tangent basis B(u) [3, 2]; boxminus returns
B(u)^T log_u(v), boxplus is exp_u(B(u) d), the noise is Q2 = B^T Q B at the predicted direction.  S and nu are lifted to the
ambient frame with B for the outputs.  The kernel works in the 3-dimensional embedded form without any basis; that the two
agree, and that no result depends on the basis, is what tests/test_bearing_reference.py checks.

Conventions as tests/sensor_meas_reference.py: mount = r[3] then qs[4] (x, y, z, w); point = b[3]."""
import numpy as np

import sensor_meas_reference as sr
from oracle import ukf_numpy as on
from update_reference import mean_iteration, nan_outputs, scored_update

LN_2PI = float(np.log(2.0 * np.pi))

POSE_POINT, POSE_NAV_DIRECTION, ORIENT_NAV_DIRECTION = 0, 1, 2
POSE_IDS, ORIENT_IDS = (0, 1), (2,)
NAMES = {0: "POSE_POINT", 1: "POSE_NAV_DIRECTION", 2: "ORIENT_NAV_DIRECTION"}
READS_LEVER = (0,)


def ids_of(man):
    return POSE_IDS if man is on.POSE else ORIENT_IDS


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------ the sphere
S2_UNRESOLVED2 = 2.0 ** -100   # (4 eps)^2: below it, with u.v < 0, the tangent part of v is not resolved (ukf_bearing.hpp)


def s2_log(u, v):
    """log_u(v) [..., 3] for unit u, v: theta t / |t|, t = v - (u.v) u, theta = atan2(|u x v|, u.v); 0 where t = 0.  The
    kernel's definition (ukf_bearing.hpp s2_log): t is the tangent part of v - u, projected against u twice, so that the result
    is tangent over the whole range and zero to the bit at v = u; theta = atan2(|t|, u.v) (|u x v| = |t| for unit u); where
    |t| <= 4 eps is left with u.v < 0, the exact antipode included, a tangent vector of length pi (pi e x u / |e x u| for the
    axis e of e0, e1 farther from u).  NaN in, NaN out."""
    u, v = np.broadcast_arrays(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
    c = np.sum(u * v, axis=-1, keepdims=True)
    t = v - u
    t = t - np.sum(u * t, axis=-1, keepdims=True) * u
    t = t - np.sum(u * t, axis=-1, keepdims=True) * u
    nt2 = np.sum(t * t, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        nt = np.sqrt(nt2)
        w = np.where(nt2 > 0, np.arctan2(nt, c) * t / np.where(nt2 > 0, nt, 1.0), 0.0 * t)   # (t NaN: NaN)
    anti = (nt2 <= S2_UNRESOLVED2) & (c < 0)
    if anti.any():
        first = np.abs(u[..., 0:1]) < 0.6
        z = np.zeros_like(u[..., 0])
        p = np.where(first, np.stack([z, -u[..., 2], u[..., 1]], axis=-1), np.stack([u[..., 2], z, -u[..., 0]], axis=-1))
        w = np.where(anti, np.pi * p / np.linalg.norm(p, axis=-1, keepdims=True), w)
    return w


def s2_exp(u, w):
    """exp_u(w) = cos|w| u + sinc|w| w, renormalised"""
    u, w = np.broadcast_arrays(np.asarray(u, dtype=np.float64), np.asarray(w, dtype=np.float64))
    th = np.linalg.norm(w, axis=-1, keepdims=True)
    sinc = np.where(th > 1e-8, np.sin(th) / np.where(th > 0, th, 1.0), 1.0 - th * th / 6.0)
    return unit(np.cos(th) * u + sinc * w)


def basis_duff(u):
    """an orthonormal basis [..., 3, 2] of the tangent plane at u (Duff et al., "Building an orthonormal basis, revisited")"""
    u = np.asarray(u, dtype=np.float64)
    s = np.where(u[..., 2] >= 0, 1.0, -1.0)
    a = -1.0 / (s + u[..., 2])
    b = u[..., 0] * u[..., 1] * a
    e1 = np.stack([1.0 + s * u[..., 0] ** 2 * a, s * b, -s * u[..., 0]], axis=-1)
    e2 = np.stack([b, s + u[..., 1] ** 2 * a, -u[..., 1]], axis=-1)
    return np.stack([e1, e2], axis=-1)


def basis_rotated(angle):
    """basis_duff turned by `angle` in the tangent plane"""
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s], [s, c]])
    return lambda u: basis_duff(u) @ R


class S2:
    """the unit sphere with a tangent basis, in the interface of oracle.ukf_numpy._Compound (D, boxplus, boxminus)"""
    D = 2
    S = 3

    def __init__(self, basis=basis_duff):
        self.basis = basis

    def boxminus(self, x, y):
        x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        return np.einsum("...ij,...i->...j", self.basis(y), s2_log(y, x))

    def boxplus(self, x, d, scale=1.0):
        return s2_exp(x, np.einsum("...ij,...j->...i", self.basis(x), scale * np.asarray(d, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------ the models
def direction(mid, X, mount, point):
    """d(X) [..., 3] before it is normalised; mount [..., 7], point [..., 3] broadcast against X's leading axes"""
    r, qs, b = mount[..., 0:3], mount[..., 3:7], point
    if mid == POSE_POINT:
        return sr.rot_t(qs, sr.rot_t(X[..., 3:7], b - X[..., 0:3]) - r)
    q = X[..., 3:7] if mid == POSE_NAV_DIRECTION else X[..., 0:4]
    return sr.rot_t(qs, sr.rot_t(q, np.broadcast_to(b, q.shape[:-1] + (3,))))


def used_inputs(mid):
    """(entries of mount [7], entries of point [3]) that model `mid` reads; every model reads all of z and Q"""
    mm = np.ones(7, bool)
    mm[0:3] = mid in READS_LEVER
    return mm, np.ones(3, bool)


mean_steps = mean_iteration   # (trips [B], norms [B, trips.max() + 1]) of the mean on the sphere


def update_bearing(man, mu, cov, models, z, Q, mount, point, gate_chi2=-1.0, initialised=None, tol=on.MEAN_TOL,
                   max_it=on.MEAN_MAX_IT, basis=basis_duff):
    """mu [B, S], cov [B, D, D], models an int or [B], z [B, 3], Q [B, 3, 3] (or [3, 3]), mount [B, 7] (or [7]), point [B, 3]
    (or [3]) -> dict(mu, cov, z_pred [B, 3], S [B, 3, 3], innov [B, 3], maha [B], loglik [B], status [B]) and, for the tests'
    own assertions, trips [B] (mean steps above tol), spread [B] (the largest sigma-point angle from z-bar), logdet [B] and
    tol_margin [B] (the smallest relative distance of a mean step's norm from tol); NaN / 0 for filters that were not scored."""
    B = mu.shape[0]
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    z = np.asarray(z, dtype=np.float64)
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, 3, 3))
    mount = np.broadcast_to(np.asarray(mount, dtype=np.float64), (B, 7))
    point = np.broadcast_to(np.asarray(point, dtype=np.float64), (B, 3))
    init = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    manz = S2(basis)
    o = dict(nan_outputs(mu, cov, 3, 3), trips=np.zeros(B, np.int64), spread=np.full(B, np.nan), logdet=np.full(B, np.nan),
             tol_margin=np.full(B, np.nan))
    valid = np.isin(models, ids_of(man))
    o["status"][~init] = on.ST_UNINITIALISED
    o["status"][init & ~valid] = on.ST_INACTIVE
    for mid in np.unique(models[init & valid]):
        mid = int(mid)
        idx = np.nonzero(init & valid & (models == mid))[0]
        um, up = used_inputs(mid)
        with np.errstate(over="ignore", invalid="ignore"):
            zz = np.sum(z[idx] * z[idx], axis=1)
        fin = (np.isfinite(z[idx]).all(axis=1) & np.isfinite(Q[idx]).all(axis=(1, 2)) & np.isfinite(mount[idx][:, um]).all(axis=1) &
               np.isfinite(point[idx][:, up]).all(axis=1) & np.isfinite(zz) & (zz > 0))
        o["status"][idx[~fin]] = on.ST_ERR_NONFINITE_MEAS
        idx = idx[fin]
        if idx.size == 0:
            continue
        zhat = unit(z[idx])
        Ql = np.tril(Q[idx])
        Q3 = Ql + np.swapaxes(np.tril(Q[idx], -1), 1, 2)   # symmetric from the lower triangle
        # entries the model does not read never meet arithmetic
        mt = np.where(um, mount[idx], sr.IDENTITY_MOUNT)[:, None, :]
        pt = point[idx][:, None, :]
        ok = _pd(cov[idx])
        sig = np.where(ok[:, None, None], cov[idx], np.eye(man.D))
        X, _ = on.sigma_points(man, mu[idx], sig)
        d = direction(mid, X, mt, pt)
        with np.errstate(over="ignore", invalid="ignore"):
            d2n = np.sum(d * d, axis=-1)
        degen = ~(np.isfinite(d2n) & (d2n > 0)).all(axis=1)   # a sigma point with |d|^2 zero or not finite: S is not finite
        safe = np.array([1.0, 0.0, 0.0])

        def hh(Xs, degen=degen, mt=mt, pt=pt, mid=mid):
            dd = direction(mid, Xs, mt if Xs.ndim == 3 else mt[:, 0], pt if Xs.ndim == 3 else pt[:, 0])
            sel = degen[:, None, None] if Xs.ndim == 3 else degen[:, None]
            return unit(np.where(sel, safe, dd))

        def Q2(mz, Q3=Q3):
            Bz = basis(mz)
            return np.swapaxes(Bz, 1, 2) @ Q3 @ Bz
        # Sigma is judged here, on the matrix as given; a failed one goes in as the identity and fails through extra_fail
        u = scored_update(man, manz, mu[idx], sig, zhat, hh, Q2, tol, max_it, gate_chi2, extra_fail=degen | ~ok)
        # No sigma points, no mean: the kernels set the bit only where Sigma factorised (do_u && ok1 && !conv).  Stated here
        # and not in the core, which returns what the other three references have always returned: on S^2 the identity that
        # stands in for a failed Sigma spreads the points by a radian and the mean really iterates; no test of the others pairs
        # a failed Sigma with a capped mean.
        s = np.where(ok, u.status, u.status & ~np.uint32(on.ST_WARN_MEAN_NOCONV)).astype(np.uint32)
        trips, steps = mean_steps(manz, u.Z, tol, max_it)
        Bz, scored = basis(u.mz), u.scored
        o["mu"][idx[u.commit]], o["cov"][idx[u.commit]] = u.mu2[u.commit], u.cov2[u.commit]
        sc = idx[scored]
        o["z_pred"][sc] = u.mz[scored]
        o["S"][sc] = (Bz @ u.S @ np.swapaxes(Bz, 1, 2))[scored]
        o["innov"][sc] = np.einsum("bij,bj->bi", Bz, u.innov)[scored]
        o["maha"][sc] = u.d2[scored]
        o["logdet"][sc] = u.logdet[scored]
        o["loglik"][sc] = -0.5 * (u.d2[scored] + u.logdet[scored] + 2.0 * LN_2PI)
        o["trips"][sc] = trips[scored]
        o["spread"][sc] = np.max(np.linalg.norm(s2_log(u.mz[:, None, :], u.Z), axis=-1), axis=1)[scored]
        o["tol_margin"][sc] = np.nanmin(np.abs(steps - tol) / tol, axis=1)[scored]
        o["status"][idx] = s
    return o


def _pd(cov):
    return on.cholesky_lower(cov)[1]


# ------------------------------------------------------------------------------------------------ the tests' input family
def make_inputs(man, mu, lo, hi, dtype=np.float64, seed=5):
    """-> (mount [n, 7], point [n, 3], {id: z [n, 3]}, Q [n, 3, 3]) as an engine of storage `dtype` holds them: mounts
    r ~ U(-1, 1)^3, qs = exp(U(-1, 1)^3); points lo ... hi metres from the body origin (OrientationState: a nav-frame vector of
    that length); z = unit(h(mu) + 0.01 N(0, 1)) U(0.5, 2), so that the normalisation is exercised; Q = 0.01^2 (I + 0.3 A A^T)"""
    n = mu.shape[0]
    rng = np.random.default_rng(seed)
    st = lambda x: np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)   # noqa: E731
    mount = np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)), on.so3_exp(rng.uniform(-1.0, 1.0, (n, 3)))], axis=1)
    away = unit(rng.standard_normal((n, 3))) * rng.uniform(lo, hi, (n, 1))
    point = (mu[:, 0:3] + away) if man is on.POSE else away
    mount, point = st(mount), st(point)
    z = {}
    for mid in ids_of(man):
        mt = np.where(used_inputs(mid)[0], mount, sr.IDENTITY_MOUNT)
        z[mid] = st(unit(unit(direction(mid, mu, mt, point)) + 0.01 * rng.standard_normal((n, 3))) * rng.uniform(0.5, 2.0, (n, 1)))
    A = rng.standard_normal((n, 3, 3))
    Q = st(0.01 ** 2 * (np.eye(3) + 0.3 * A @ np.swapaxes(A, 1, 2)))
    return mount, point, z, Q
