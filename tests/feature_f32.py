"""The five feature calls (innovation statistics, state-block and sensor-frame measurements, the backward step of the smoother,
the mixture moments of a filter bank) with a dtype per STAGE, assembled from the stage functions of tests/study_f32_mixed.py
(Prec, sigma_points, manifold_mean, chol, the process models, the SO(3) maps).  A helper, not collected;
tests/test_feature_scaled_reference.py pins it: with every stage float64 it is the float64 reference of each family to 1e-12,
with every stage float32 it is the `d_32` of tests/feature_scaled_parity.py, the drift a correct fp32 evaluation of the same
algorithm shows on the same batch.  kernel_ident is off (as scaled_parity.fp32_spread): no stage uses the engine's exact
identities, so that the spread of a correct fp32 evaluation is not understated.

Beyond predict / update of the study this file adds: measurement manifolds with any number of SO(3) blocks (Fields), the eight
sensor models (tests/sensor_meas_reference.h, evaluated in float64 in every mode as the kernel does), the
cross-covariance, gain and Jr^-1 transport of the backward step, and the weighted manifold mean and spread of means of the
bank.  The shaped process noise of a backward step (a rotation of two 3x3 blocks and a scale) is taken from the reference in
float64 and rounded to the linear-algebra dtype once.

Status handling is the caller's: every function here computes every row and expects inputs that factorise; rows the reference
does not commit are put back by `keep`."""
import numpy as np

import study_f32_mixed as st
from study_f32_mixed import F32, F64, Prec

P64 = Prec("f64", F64, F64, F64, kernel_ident=False)
P32 = Prec("f32", F32, F32, F32, kernel_ident=False)
PRECISIONS = {"f64": P64, "f32": P32}


class Fields:
    """a compound of vector and SO(3) blocks with the interface of study_f32_mixed.Man (S, D, plus, minus); fields as
    oracle.ukf_numpy._Compound: (kind, stored offset, tangent offset, dim)"""

    def __init__(self, fields):
        self.fields = list(fields)
        self.S = sum(4 if k == "so3" else n for k, _, _, n in self.fields)
        self.D = sum(3 if k == "so3" else n for k, _, _, n in self.fields)

    def plus(self, x, d):
        out = np.array(np.broadcast_to(x, np.broadcast_shapes(x.shape[:-1], d.shape[:-1]) + (self.S,)))
        for kind, so, to, n in self.fields:
            if kind == "so3":
                out[..., so:so + 4] = st.qmul(out[..., so:so + 4], st.so3_exp(d[..., to:to + 3]))
            else:
                out[..., so:so + n] = out[..., so:so + n] + d[..., to:to + n]
        return out

    def minus(self, x, y):
        d = np.empty(np.broadcast_shapes(x.shape[:-1], y.shape[:-1]) + (self.D,), dtype=x.dtype)
        for kind, so, to, n in self.fields:
            if kind == "so3":
                d[..., to:to + 3] = st.so3_log(st.qmul(st.qconj(y[..., so:so + 4]), x[..., so:so + 4]))
            else:
                d[..., to:to + n] = x[..., so:so + n] - y[..., so:so + n]
        return d


def vect(m):
    return Fields([("vec", 0, 0, m)])


SO3 = Fields([("so3", 0, 0, 3)])
STATE = {"pose": Fields([("vec", 0, 0, 3), ("so3", 3, 3, 3), ("vec", 7, 6, 3), ("vec", 10, 9, 3)]),
         "orient": Fields([("so3", 0, 0, 3), ("vec", 4, 3, 3), ("vec", 7, 6, 3), ("vec", 10, 9, 3), ("vec", 13, 12, 1)])}
ROT = {"pose": 3, "orient": 0}   # tangent offset of the rotation


def sub_fields(model, mask):
    """-> (the compound of the state blocks `mask` selects, their stored indices, their tangent indices)"""
    fields, stored, tangent, so, to = [], [], [], 0, 0
    for b, (kind, s0, t0, n) in enumerate(STATE[model].fields):
        if (int(mask) >> b) & 1:
            ns, nt = (4, 3) if kind == "so3" else (n, n)
            fields.append((kind, so, to, n))
            stored += list(range(s0, s0 + ns))
            tangent += list(range(t0, t0 + nt))
            so, to = so + ns, to + nt
    return Fields(fields), np.array(stored), np.array(tangent)


def _outer_sum(a, b):
    return np.einsum("bia,bic->bac", a, b)


def manifold_mean(man, X0, Xp, Xm, P):
    """study_f32_mixed.manifold_mean for points that live on another manifold than the state (it takes the number of points
    from man.D): reference = X0, mean of the deltas in tm until its norm <= 1e-6, the reference's own steps in tc"""
    ref = X0.copy()
    n = 2 * Xp.shape[1] + 1
    active = np.ones(ref.shape[0], dtype=bool)
    for _ in range(100):
        refm = ref.astype(P.tm)[:, None, :]
        d = (man.minus(Xp, refm).sum(1) + man.minus(Xm, refm).sum(1) + man.minus(X0.astype(P.tm), refm[:, 0])) / P.tm(n)
        ref = np.where(active[:, None], man.plus(ref, d.astype(P.tc)), ref)
        active = active & (np.sqrt((d.astype(F64) ** 2).sum(-1)) > st.MEAN_TOL)
        if not active.any():
            break
    return ref


# ------------------------------------------------------------------------------------------------ measurement statistics, update
def statistics(man, manz, mu, cov, h, Q, P):
    """-> dict(L, zbar [B, Sz], S [B, m, m], Cxz [B, D, m]) in (tl, tm, tl, tl): the sigma points of (mu, cov) through h"""
    cov = cov.astype(P.tl)
    L = st.chol(cov)
    X0, Xp, Xm = st.sigma_points(man, mu, L, P)
    Z0, Zp, Zm = h(X0.astype(P.tm)), h(Xp), h(Xm)
    zbar = manifold_mean(manz, Z0, Zp, Zm, P)
    zm = zbar.astype(P.tm)[:, None, :]
    dzp, dzm = manz.minus(Zp, zm).astype(P.tl), manz.minus(Zm, zm).astype(P.tl)
    dz0 = manz.minus(Z0, zm[:, 0]).astype(P.tl)
    S = 0.5 * (_outer_sum(dzp, dzp) + _outer_sum(dzm, dzm) + dz0[:, :, None] * dz0[:, None, :]) + Q.astype(P.tl)
    cols = np.swapaxes(L, 1, 2)                                   # state deltas: (mu (+) d) (-) mu = d, the centre's is 0
    Cxz = 0.5 * (_outer_sum(cols, dzp) - _outer_sum(cols, dzm))
    return dict(cov=cov, zbar=zbar, S=S, Cxz=Cxz)


def innovation(manz, z, zbar, P):
    return manz.minus(z.astype(P.tm), zbar.astype(P.tm)).astype(P.tl)


def apply_delta(man, mu, cov2, delta, P):
    """ukfom's applyDelta: the sigma points of (mu, cov2) shifted by delta, their centre and their spread about it"""
    L2 = st.chol(cov2)
    X0, Xp, Xm = st.sigma_points(man, mu, L2, P, delta)
    mm = X0.astype(P.tm)[:, None, :]
    dp, dm = man.minus(Xp, mm).astype(P.tl), man.minus(Xm, mm).astype(P.tl)
    return X0, 0.5 * (_outer_sum(dp, dp) + _outer_sum(dm, dm))


def update(man, manz, mu, cov, z, h, Q, P):
    """-> dict(mu, cov, z_pred, S, innov) as an engine of storage P.ts returns them, in float64"""
    s = statistics(man, manz, mu, cov, h, Q, P)
    nu = innovation(manz, z, s["zbar"], P)
    K = s["Cxz"] @ np.linalg.inv(s["S"])
    cov2 = s["cov"] - K @ s["S"] @ np.swapaxes(K, 1, 2)
    cov2 = 0.5 * (cov2 + np.swapaxes(cov2, 1, 2))
    m2, C2 = apply_delta(man, mu, cov2, (K @ nu[:, :, None])[:, :, 0], P)
    o = lambda x: x.astype(P.ts).astype(F64)   # noqa: E731
    return dict(mu=o(m2), cov=o(C2), z_pred=o(s["zbar"]), S=o(s["S"]), innov=o(nu))


def state_meas(model, mu, cov, masks, z, Qz, a=1.0, b=1.0, keep=None, prec="f32"):
    """The joint state-block measurement (tests/state_meas_reference.update_state) -> (mu [B, S], cov [B, D, D]).  Rows with
    an invalid mask, and rows where `keep` [B] is set (gated, failed), return the state they came with."""
    P, man = PRECISIONS[prec], STATE[model]
    B = mu.shape[0]
    masks = np.broadcast_to(np.asarray(masks, dtype=np.int64), (B,))
    keep = np.zeros(B, bool) if keep is None else np.asarray(keep, dtype=bool)
    mu_o, cov_o = np.array(mu, dtype=F64), np.array(cov, dtype=F64)
    valid = (masks > 0) & ((masks >> len(man.fields)) == 0) & ~keep
    for m in np.unique(masks[valid]):
        idx = np.nonzero(valid & (masks == m))[0]
        manz, si, ti = sub_fields(model, m)
        sig = (P.tl(a) * cov[idx].astype(P.tl)).astype(P.ts)   # (a no-op for a = 1)
        QQ = P.tl(b) * Qz[idx][:, ti[:, None], ti[None, :]].astype(P.tl)
        r = update(man, manz, mu[idx].astype(P.ts), sig, z[idx][:, si].astype(P.ts), lambda X: X[..., si], QQ, P)
        mu_o[idx], cov_o[idx] = r["mu"], r["cov"]
    return mu_o, cov_o


def sensor_meas(model, mu, cov, ids, z, Q, mount, point, gyro=None, keep=None, prec="f32"):
    """The sensor-frame measurement (tests/sensor_meas_reference.update_sensor) -> dict(mu, cov, z_pred [B, 3], S [B, 3, 3],
    innov [B, 3]); outputs of rows without a model of this engine are NaN, their state and that of `keep` rows is unchanged"""
    import sensor_meas_reference as smr
    P, man = PRECISIONS[prec], STATE[model]
    B = mu.shape[0]
    ids = np.broadcast_to(np.asarray(ids, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=F64), (B, 3, 3))
    mount = np.broadcast_to(np.asarray(mount, dtype=F64), (B, 7))
    point = np.broadcast_to(np.asarray(point, dtype=F64), (B, 3))
    gyro = np.zeros((B, 3)) if gyro is None else np.asarray(gyro, dtype=F64)
    keep = np.zeros(B, bool) if keep is None else np.asarray(keep, dtype=bool)
    o = dict(mu=np.array(mu, dtype=F64), cov=np.array(cov, dtype=F64), z_pred=np.full((B, 3), np.nan), S=np.full((B, 3, 3), np.nan),
             innov=np.full((B, 3), np.nan))
    own = smr.POSE_IDS if model == "pose" else smr.ORIENT_IDS
    for mid in np.unique(ids[np.isin(ids, own)]):
        mid = int(mid)
        m = smr.meas_dim(mid)
        idx = np.nonzero(ids == mid)[0]
        _, _, um, up = smr.used_inputs(mid)
        mt = np.where(um, mount[idx], smr.IDENTITY_MOUNT)[:, None, :]
        pt = np.where(up, point[idx], 0.0)[:, None, :]
        gy = gyro[idx][:, None, :]

        def hh(X):   # float64 in every mode: the kernel evaluates the sensor models in double
            one = X.ndim == 2
            return smr.h(mid, X.astype(F64), mt[:, 0] if one else mt, pt[:, 0] if one else pt, gy[:, 0] if one else gy).astype(X.dtype)
        r = update(man, vect(m), mu[idx].astype(P.ts), cov[idx].astype(P.ts), z[idx][:, :m].astype(P.ts), hh, Q[idx][:, :m, :m], P)
        go = ~keep[idx]
        o["mu"][idx[go]], o["cov"][idx[go]] = r["mu"][go], r["cov"][go]
        o["z_pred"][idx], o["S"][idx], o["innov"][idx] = 0.0, 0.0, 0.0
        o["z_pred"][idx, :m], o["innov"][idx, :m] = r["z_pred"], r["innov"]
        o["S"][idx[:, None, None], np.arange(m)[None, :, None], np.arange(m)[None, None, :]] = r["S"]
    return o


POSE_SELECT = {0: [0, 1, 2], 1: [0, 1], 2: [2], 4: [7, 8, 9], 5: [7, 8], 6: [9], 7: [7, 12], 8: [10, 11, 12]}


def cycle_model(kind, mid):
    """(m, measurement manifold, h) of the cycle kernels' measurement model `mid` (include/ukf_batch.h); 3 = ORIENT_SO3"""
    if kind == "orient":
        return 3, vect(3), lambda X: st.qrot(st.qinv(X[..., 0:4]), X[..., 4:7])
    if mid == 3:
        return 3, SO3, lambda X: X[..., 3:7]
    idx = POSE_SELECT[mid]
    return len(idx), vect(len(idx)), lambda X: X[..., idx]


def innovation_stats(kind, mid, mu, cov, Q, z, prec="f32"):
    """The innovation call -> (zbar [B, Sz], S [B, m, m], nu [K, B, m]) of candidates z [K, B, 3] (axis-angle for model 3)"""
    P = PRECISIONS[prec]
    m, manz, h = cycle_model(kind, mid)
    s = statistics(STATE[kind], manz, mu.astype(P.ts), cov.astype(P.ts), h, Q[:, :m, :m], P)
    nu = []
    for k in range(z.shape[0]):
        zk = st.so3_exp(z[k].astype(P.tm)) if manz is SO3 else z[k][:, :m]
        nu.append(innovation(manz, zk, s["zbar"], P))
    o = lambda x: x.astype(P.ts).astype(F64)   # noqa: E731
    return o(s["zbar"]), o(s["S"]), o(np.array(nu))


def cycle_update(kind, mid, mu, cov, z, Q, prec="f32"):
    """ukfb_update_dev with a uniform model id -> (mu, cov): the second fp32 evaluation behind M_feat"""
    P = PRECISIONS[prec]
    m, manz, h = cycle_model(kind, mid)
    zz = st.so3_exp(z.astype(P.tm)) if manz is SO3 else z[:, :m]
    r = update(STATE[kind], manz, mu.astype(P.ts), cov.astype(P.ts), zz.astype(P.ts), h, Q[:, :m, :m], P)
    return r["mu"], r["cov"]


# ------------------------------------------------------------------------------------------------ the smoother's backward step
def jr_inv(p):
    """Jr^-1(phi) = I + [phi]x / 2 + c(theta) [phi]x^2 (tests/bank_reference.jr_inv) in the dtype of p"""
    t = p.dtype.type
    th = np.sqrt((p * p).sum(-1))
    small = th < t(1e-2)
    h = t(0.5) * np.where(small, t(1), th)
    c = np.where(small, t(1.0 / 12.0) + th * th * t(1.0 / 720.0), (np.sin(h) - h * np.cos(h)) / (t(4) * h * h * np.sin(h)))
    H = np.zeros(p.shape[:-1] + (3, 3), dtype=p.dtype)
    H[..., 0, 1], H[..., 0, 2] = -p[..., 2], p[..., 1]
    H[..., 1, 0], H[..., 1, 2] = p[..., 2], -p[..., 0]
    H[..., 2, 0], H[..., 2, 1] = -p[..., 1], p[..., 0]
    return np.eye(3, dtype=p.dtype) + t(0.5) * H + c[..., None, None] * (H @ H)


def backward_step(p, mu, cov, mu_s, cov_s, dt, in_a, in_b, P):
    """(mu, cov) filtered at c in ts, (mu_s, cov_s) the chain at c + 1 in (tc, tl) -> the chain at c in (tc, tl)"""
    import smoother_reference as smr
    model = p.model
    man, ro, D = STATE[model], ROT[model], STATE[model].D
    B = mu.shape[0]
    _, R = smr._process_and_noise(p, mu.astype(F64), dt, in_a, in_b)
    bc = lambda a, X: (a[:, None, :] if X.ndim == 3 else a).astype(X.dtype)   # noqa: E731
    if model == "pose":
        use = np.zeros(B, bool) if in_a is None else np.isfinite(in_a).all(axis=-1)
        acc = np.where(use[:, None], np.zeros((B, 3)) if in_a is None else in_a, 0.0)
        g = lambda X: st.pose_process(X, bc(acc, X), dt)                     # noqa: E731
    else:
        assert p.tau_g == p.tau_a
        g = lambda X: st.orient_process(X, bc(in_a, X), bc(in_b, X), p.tau_g, p.earth.astype(X.dtype), dt)   # noqa: E731
    cov = cov.astype(P.tl)
    L = st.chol(cov)
    X0, Xp, Xm = st.sigma_points(man, mu, L, P)
    Y0, Yp, Ym = g(X0), g(Xp), g(Xm)
    m_pred = st.manifold_mean(man, Y0, Yp, Ym, P)
    mm = m_pred.astype(P.tm)[:, None, :]
    dp, dm = man.minus(Yp, mm).astype(P.tl), man.minus(Ym, mm).astype(P.tl)
    d0 = man.minus(Y0.astype(P.tm), mm[:, 0]).astype(P.tl)
    Cp = 0.5 * (_outer_sum(dp, dp) + _outer_sum(dm, dm) + d0[:, :, None] * d0[:, None, :]) + R.astype(P.tl)
    cols = np.swapaxes(L, 1, 2)
    C = 0.5 * (_outer_sum(cols, dp) - _outer_sum(cols, dm))
    G = np.swapaxes(np.linalg.solve(Cp, np.swapaxes(C, 1, 2)), 1, 2)
    e = man.minus(mu_s.astype(P.tm), m_pred.astype(P.tm)).astype(P.tl)
    J = np.broadcast_to(np.eye(D, dtype=P.tl), (B, D, D)).copy()
    J[:, ro:ro + 3, ro:ro + 3] = jr_inv(e[:, ro:ro + 3])
    St = J @ cov_s.astype(P.tl) @ np.swapaxes(J, 1, 2)
    Sig = cov + G @ (St - Cp) @ np.swapaxes(G, 1, 2)
    Sig = np.tril(Sig) + np.swapaxes(np.tril(Sig, -1), 1, 2)
    return apply_delta(man, mu, Sig, (G @ e[:, :, None])[:, :, 0], P)


def smooth(p, mu, cov, dt, in_a=None, in_b=None, rows=None, prec="f32"):
    """tests/smoother_reference.smooth for the filters `rows` -> (mu_s [steps, B, S], cov_s [steps, B, D, D]) as an engine of
    storage P.ts writes them (the chain itself is never narrowed below the arithmetic dtype: ukf_smooth.hpp keeps CSM / CSP
    in T and narrows each step's record once).  A step with dt <= min_dt copies the step above."""
    P = PRECISIONS[prec]
    rows = slice(None) if rows is None else rows
    mu, cov = np.asarray(mu, dtype=F64)[:, rows], np.asarray(cov, dtype=F64)[:, rows]
    steps = mu.shape[0]
    dt = np.asarray(dt, dtype=F64).reshape(steps - 1)
    ring = lambda x, c: None if x is None else (x[c][rows] if np.ndim(x) == 3 else x[rows])   # noqa: E731
    import copy
    p = copy.copy(p)
    if np.ndim(p.R) == 3:
        p.R = p.R[rows]
    mu_s, cov_s = mu.copy(), cov.copy()
    m, C = mu[-1].astype(P.tc), cov[-1].astype(P.tl)
    for c in range(steps - 2, -1, -1):
        if dt[c] > p.min_dt:
            m, C = backward_step(p, mu[c].astype(P.ts), cov[c].astype(P.ts), m, C, float(dt[c]), ring(in_a, c), ring(in_b, c), P)
        mu_s[c], cov_s[c] = m.astype(P.ts).astype(F64), C.astype(P.ts).astype(F64)
    return mu_s, cov_s


# ------------------------------------------------------------------------------------------------ filter banks
def mixture(model, mu, cov, w, prec="f32", tol=1e-6, max_it=10000):
    """tests/bank_reference.mixture (every weight > 0) -> (mean [T, S], cov [T, D, D]) in float64 as stored in P.ts: the
    weighted manifold mean from the heaviest hypothesis, and sum w_j (J_j C_j J_j^T + d_j d_j^T) about it"""
    P, man, ro = PRECISIONS[prec], STATE[model], ROT[model]
    T, M, _ = mu.shape
    D = man.D
    mus, w_m, w_l = mu.astype(P.ts), w.astype(P.tm), w.astype(P.tl)
    ref = mus[np.arange(T), np.argmax(w, axis=1)].astype(P.tc)
    active, it = np.ones(T, bool), np.zeros(T, np.int64)
    while active.any():
        d = np.zeros((T, D), dtype=P.tm)
        for j in range(M):
            d = d + w_m[:, j, None] * man.minus(mus[:, j].astype(P.tm), ref.astype(P.tm))
        norm = np.sqrt((d.astype(F64) ** 2).sum(-1))
        ref = np.where(active[:, None], man.plus(ref, d.astype(P.tc)), ref)
        big = norm > tol
        it = np.where(active & big, it + 1, it)
        active = active & big & (it < max_it)
    C = np.zeros((T, D, D), dtype=P.tl)
    for j in range(M):
        dj = man.minus(mus[:, j].astype(P.tm), ref.astype(P.tm)).astype(P.tl)
        J = np.broadcast_to(np.eye(D, dtype=P.tl), (T, D, D)).copy()
        J[:, ro:ro + 3, ro:ro + 3] = jr_inv(dj[:, ro:ro + 3])
        C = C + w_l[:, j, None, None] * (J @ cov[:, j].astype(P.tl) @ np.swapaxes(J, 1, 2) + dj[:, :, None] * dj[:, None, :])
    return ref.astype(P.ts).astype(F64), C.astype(P.ts).astype(F64)


def mix(model, mu, cov, w, Pi, prec="f32", **kw):
    """tests/bank_reference.mix (every c_i > 0) -> (mu' [T, M, S], cov' [T, M, D, D]); the mixing weights in the
    linear-algebra dtype"""
    P = PRECISIONS[prec]
    wl, Pl = w.astype(P.tl), np.asarray(Pi).astype(P.tl)
    c = wl @ Pl
    wji = (Pl.T[None, :, :] * wl[:, None, :]) / c[:, :, None]
    out = [mixture(model, mu, cov, wji[:, i].astype(F64), prec, **kw) for i in range(mu.shape[1])]
    return np.stack([o[0] for o in out], axis=1), np.stack([o[1] for o in out], axis=1)
