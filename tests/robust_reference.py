"""NumPy float64 statement of the robust sensor-frame update of include/ukf_batch_robust.h: a robust update with scale lambda
IS sensor_meas_reference.update_sensor with lambda Q, so this file adds only the scale -- solve_scale, the root of
d^2(lambda) = c^2 by bracketing and bisection (independent of Newton), newton_iterates, the kernel's rule restated with every
iterate kept -- and update_robust, which puts the header's zones and statuses around the two.  A helper, not collected;
tests/test_robust_reference.py pins it.

Everything works on the measurement side embedded in R^3 as the kernel embeds it: Sigma_z is the identity beyond m, Q and nu
are zero there, so that rows of m = 1 and m = 3 go through one vectorised path."""
import collections

import numpy as np

import sensor_meas_reference as sr
from oracle import ukf_numpy as on

MATCH, HUBER = 0, 1
CHI2_M1, CHI2_M3 = 3.8415, 7.8147   # chi^2_0.95 of 1 and 3 degrees of freedom
Rule = collections.namedtuple("Rule", "mode chi2_m1 chi2_m3 scale_max tol max_iter")
FLOAT_KEYS = ("z_pred", "S", "innov", "maha0", "maha", "loglik", "scale")


def rule(mode=MATCH, chi2_m1=CHI2_M1, chi2_m3=CHI2_M3, scale_max=1e30, tol=1e-13, max_iter=16):
    return Rule(int(mode), float(chi2_m1), float(chi2_m3), float(scale_max), float(tol), int(max_iter))


def thresholds(models, r):
    """c^2 per row by the model's m (rows without a model: chi2_m3, never used)"""
    return np.where(np.asarray(models) == sr.POSE_RANGE, r.chi2_m1, r.chi2_m3)


def embed(models, S, Q, nu):
    """the outputs S [B, 3, 3] (zero outside the leading m x m), nu [B, 3] of an update at lambda = 1 and its Q [B, 3, 3]
    -> (Sigma_z, Q, nu) embedded: the identity, zero, zero beyond m"""
    m = np.where(np.asarray(models) == sr.POSE_RANGE, 1, 3)
    inside = (np.arange(3)[None, :] < m[:, None])
    blk = inside[:, :, None] & inside[:, None, :]
    Qe = np.where(blk, Q, 0.0)
    Sz = np.where(blk, S - Qe, np.eye(3))
    return Sz, Qe, np.where(inside, nu, 0.0)


def evaluate(Sz, Q, nu, lam, dtype=np.float64):
    """-> f = d^2(lambda) = nu^T S(lambda)^-1 nu and g = x^T Q x, x = S(lambda)^-1 nu (-g is df / dlambda), per row"""
    lam = np.asarray(lam, dtype=dtype)
    S = (Sz + lam[:, None, None] * Q).astype(dtype)
    x = np.linalg.solve(S, nu.astype(dtype)[:, :, None])[:, :, 0].astype(dtype)
    f = np.einsum("bi,bi->b", nu.astype(dtype), x).astype(dtype)
    g = np.einsum("bi,bij,bj->b", x, Q.astype(dtype), x).astype(dtype)
    return f, g


def solve_scale(Sz, Q, nu, c2, mode):
    """lambda per row for rows that are all outliers (d^2(1) > c^2), float64.  HUBER: the closed form.  MATCH: the root of
    d^2(lambda) = c^2 by doubling a bracket from [1, 2] and bisecting it in ln lambda; Newton is not involved"""
    c2 = np.broadcast_to(np.asarray(c2, dtype=np.float64), (Sz.shape[0],))
    f0, _ = evaluate(Sz, Q, nu, np.ones(Sz.shape[0]))
    assert (f0 > c2).all()
    if mode == HUBER:
        return np.sqrt(f0 / c2)
    lo, hi = np.ones(Sz.shape[0]), np.full(Sz.shape[0], 2.0)
    for _ in range(200):
        above = evaluate(Sz, Q, nu, hi)[0] > c2
        if not above.any():
            break
        lo, hi = np.where(above, hi, lo), np.where(above, 2.0 * hi, hi)
    assert not above.any(), "no bracket: Q is not positive definite on some row"
    for _ in range(200):
        mid = np.sqrt(lo * hi)
        above = evaluate(Sz, Q, nu, mid)[0] > c2
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    return np.sqrt(lo * hi)


def newton_iterates(Sz, Q, nu, c2, tol=1e-13, max_iter=16, scale_max=1e30, dtype=np.float64):
    """The kernel's rule for rows that are all outliers: Newton on 1 / d^2 - 1 / c^2 from lambda = 1, every row stopping on the
    first of f - c^2 <= tol c^2, a step that does not increase lambda, g not positive or not finite, lambda >= scale_max,
    max_iter steps.  -> (iterates [B, steps.max() + 1] with a row's last value repeated beyond its own steps, steps [B]).
    The clamp to scale_max is not applied.  dtype: the arithmetic (float32 for the bound of a plain fp32 engine)."""
    t = dtype
    B = Sz.shape[0]
    c2 = np.broadcast_to(np.asarray(c2, dtype=t), (B,))
    tol, scale_max = t(tol), t(scale_max)
    lam, its = np.ones(B, dtype=t), np.zeros(B, dtype=np.int64)
    f, g = evaluate(Sz, Q, nu, lam, t)
    active = f - c2 > tol * c2
    out = [lam.copy()]
    with np.errstate(all="ignore"):
        while active.any():
            lam_new = (lam + f * (f - c2) / (c2 * g)).astype(t)
            go = active & (g > 0) & np.isfinite(g) & (lam_new > lam)
            lam = np.where(go, lam_new, lam).astype(t)
            its = its + go
            f2, g2 = evaluate(Sz, Q, nu, lam, t)
            f, g = np.where(go, f2, f), np.where(go, g2, g)
            active = go & (f - c2 > tol * c2) & (lam < scale_max) & (its < max_iter)
            out.append(lam.copy())
    return np.stack(out, axis=1), its


RHO = (0.5, 1.5, 4.0, 8.0, 30.0, 300.0)   # Mahalanobis radii of the contaminated batch: filter i gets RHO[i mod 6]
GATE = 400.0                               # between rho = 8 and rho = 30
SCALE_MAX_CHOICES = (30.0, 100.0, 300.0, 1000.0)
# the models whose contaminated batch leaves a choice of scale_max with no root within 10 % of it (the roots of POSE_POINT,
# ORIENT_NAV_VECTOR and ORIENT_SPECIFIC_FORCE spread over every choice): m = 1 and m = 3 for Pose, m = 3 for OrientationState
CLAMP_MODELS = {"pose": (sr.POSE_RANGE, sr.POSE_VELOCITY), "orient": (sr.ORIENT_VELOCITY,)}


def contaminate(man, mu, cov, models, z, Q, mount, point, gyro=None, seed=7):
    """z with the innovation of filter i replaced by Ls u rho: Ls the factor of the filter's own S at lambda = 1, u a random
    unit vector, rho = RHO[i mod 6] -- a sample at Mahalanobis radius rho.  Rows that are not scored keep their z."""
    B = mu.shape[0]
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    raw = sr.update_sensor(man, mu, cov, models, z, Q, mount, point, gyro)
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((B, 3))
    out = np.array(z, dtype=np.float64, copy=True)
    rho = np.array(RHO)[np.arange(B) % len(RHO)]
    for i in np.nonzero(~np.isnan(raw["maha"]))[0]:
        m = sr.meas_dim(int(models[i]))
        Ls = np.linalg.cholesky(raw["S"][i, :m, :m])
        out[i, :m] = raw["z_pred"][i, :m] + Ls @ (u[i, :m] / np.linalg.norm(u[i, :m])) * rho[i]
    return out


def pick_scale_max(roots):
    """the first of SCALE_MAX_CHOICES that no root lies within 10 % of"""
    for s in SCALE_MAX_CHOICES:
        if not (np.abs(roots - s) <= 0.1 * s).any():
            return s
    raise AssertionError("every choice of scale_max has a root within 10 %")


def update_robust(man, mu, cov, models, z, Q, mount, point, gyro=None, rule=None, gate_chi2=-1.0, initialised=None, scale=None):
    """The arguments of sr.update_sensor and a Rule -> its dict with maha0 [B], scale [B], iterations [B] added.  The scores of
    update_sensor at lambda = 1 with the gate off; the gate on the raw distance (REJECTED_GATE: the state kept, those scores,
    iterations 0); lambda = 1 for d0^2 <= c^2, else by the rule's mode (MATCH: newton_iterates' last, the kernel's rule),
    clamped to scale_max; then update_sensor with lambda Q and the gate off.  A row the first call refuses stays refused: NaN in
    every float output, iterations 0.  scale [B]: use these lambda for the rows that commit (NaN: the rule's), to see the
    update a given lambda makes."""
    r = rule
    B = mu.shape[0]
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, 3, 3))
    raw = sr.update_sensor(man, mu, cov, models, z, Q, mount, point, gyro, gate_chi2=-1.0, initialised=initialised)
    scored = ~np.isnan(raw["maha"])
    o = dict(raw)
    o["maha0"] = raw["maha"].copy()
    o["scale"] = np.where(scored, 1.0, np.nan)
    o["iterations"] = np.zeros(B, dtype=np.int32)
    gated = scored & (gate_chi2 >= 0) & (raw["maha"] > gate_chi2)
    c2 = thresholds(models, r)
    out = scored & ~gated & (raw["maha"] > c2)
    if out.any():
        Sz, Qe, nu = embed(models[out], raw["S"][out], Q[out], raw["innov"][out])
        if r.mode == HUBER:
            lam = np.sqrt(raw["maha"][out] / c2[out])
        else:
            it, steps = newton_iterates(Sz, Qe, nu, c2[out], r.tol, r.max_iter, r.scale_max)
            lam = it[:, -1]
            o["iterations"][out] = steps
        o["scale"][out] = np.minimum(lam, r.scale_max)
    if scale is not None:
        o["scale"] = np.where(np.isnan(scale) | ~scored | gated, o["scale"], scale)
    upd = scored & ~gated
    lamq = np.where(upd, o["scale"], 1.0)[:, None, None] * Q
    fin = sr.update_sensor(man, mu, cov, models, z, lamq, mount, point, gyro, gate_chi2=-1.0, initialised=initialised)
    for k in ("mu", "cov", "z_pred", "S", "innov", "maha", "loglik", "status"):
        o[k] = np.where(upd.reshape((B,) + (1,) * (fin[k].ndim - 1)), fin[k], raw[k])
    o["mu"][gated], o["cov"][gated] = mu[gated], cov[gated]
    o["status"] = o["status"].astype(np.uint32)
    o["status"][gated] |= np.uint32(on.ST_REJECTED_GATE)
    refused = np.isnan(o["maha"])   # the first call's, and a final S(lambda) that failed
    for k in ("maha0", "scale"):
        o[k][refused] = np.nan
    o["iterations"][refused] = 0
    return o


FLOOR_F32 = 20.0 * 2.0 ** -24


def f32_distances(model, mu, cov, ids, z, Q, mount, point, gyro, r):
    """What a correct all-float32 evaluation of the same batch leaves on lambda and on the residual, for the bounds of a plain
    fp32 engine: the sensor update's statistics by tests/feature_f32.py in float32 and in float64, Sigma_z = S - Q and the
    rule (Newton, or the closed form) in the evaluation's own dtype.  -> dict(rows [B] the outliers of the float64 evaluation,
    lam32, lam64 [rows], d_lam = max |lam32 - lam64| / lam64, d_resid = max |d^2_64(lam32) - c^2| / c^2 (MATCH))"""
    import feature_f32 as ff
    B = mu.shape[0]
    ids = np.broadcast_to(np.asarray(ids, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, 3, 3))
    c2 = thresholds(ids, r)
    ev, lam = {}, {}
    for p, t in (("f64", np.float64), ("f32", np.float32)):
        e = ff.sensor_meas(model, mu, cov, ids, z, Q, mount, point, gyro, prec=p)
        own = ~np.isnan(e["S"][:, 0, 0])
        Sz, Qe, nu = embed(ids[own], e["S"][own].astype(t), Q[own].astype(t), e["innov"][own].astype(t))
        f0, _ = evaluate(Sz, Qe, nu, np.ones(int(own.sum()), dtype=t), t)
        ev[p] = (own, Sz, Qe, nu, f0)
    own, _, _, _, f0 = ev["f64"]
    out = f0 > c2[own]
    assert np.array_equal(out, ev["f32"][4] > c2[own].astype(np.float32)), "the two evaluations disagree on who is an outlier"
    for p, t in (("f64", np.float64), ("f32", np.float32)):
        _, Sz, Qe, nu, f0 = ev[p]
        if r.mode == HUBER:
            lam[p] = np.sqrt(f0[out] / c2[own][out].astype(t)).astype(np.float64)
        else:
            it, _ = newton_iterates(Sz[out], Qe[out], nu[out], c2[own][out], r.tol, r.max_iter, r.scale_max, dtype=t)
            lam[p] = it[:, -1].astype(np.float64)
    _, Sz, Qe, nu, _ = ev["f64"]
    f, _ = evaluate(Sz[out], Qe[out], nu[out], lam["f32"])
    rows = np.zeros(B, bool)
    rows[np.nonzero(own)[0][out]] = True
    return dict(rows=rows, lam32=lam["f32"], lam64=lam["f64"], d_lam=float(np.max(np.abs(lam["f32"] - lam["f64"]) / lam["f64"])),
                d_resid=float(np.max(np.abs(f - c2[own][out]) / c2[own][out])))
