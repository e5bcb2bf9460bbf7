"""NumPy float64 statement of the late sensor-frame samples of include/ukf_batch_delayed_sensor.h, composed from pieces that are
pinned elsewhere: the backward chain of tests/delayed_reference.py (backward_chain), the eight h functions, their dimensions
and the rule of reading of tests/sensor_meas_reference.py (h, meas_dim, used_inputs) and, from tests/update_reference.py, the
scored update (the statistics and which filters are scored) and the tail of an update that commits into the present through
the history (commit_through_history).  What is stated here and nowhere else: which rotation rate model 5 reads (rate_source)
and the retrodiction of the gain with the sensor-frame statistics, K = Sigma_n M_s^T (Sigma^s_s)^-1 C_z S^-1.  A helper, not
collected; tests/test_delayed_sensor_reference.py pins it.

Arrays are in WINDOW order as in delayed_reference: mu [steps, B, S], cov [steps, B, D, D], dt [steps - 1]; step n = steps - 1
of the window arrays is never read.  `delayed_sensor_f32` is the same call with a dtype per stage (tests/feature_f32.py), the
d_32 of the scaled parity."""
import contextlib
import copy

import numpy as np

from oracle import ukf_numpy as on
import delayed_reference as dr
import sensor_meas_reference as smr
from update_reference import commit_through_history, scored_update


def rate_source(lag, steps, rate=None, in_b=None, latch_b=None):
    """The rotation rate ORIENT_VELOCITY reads, [B, 3]: `rate` when given; else the rotation-rate ring's entry of step
    s = n - lag where a ring [steps, B, 3] is bound and lag >= 1; else the latch (in_b itself when it is no ring)."""
    lag = np.asarray(lag, dtype=np.int64)
    if rate is not None:
        return np.asarray(rate, dtype=np.float64)
    if in_b is not None and np.ndim(in_b) == 3:
        n = steps - 1
        s = np.clip(n - lag, 0, n)
        ring = np.asarray(in_b, dtype=np.float64)[s, np.arange(lag.shape[0])]
        use = (lag >= 1) & (lag <= n)
        return np.where(use[:, None], ring, np.asarray(latch_b, dtype=np.float64))
    return np.asarray(in_b if latch_b is None else latch_b, dtype=np.float64)


def update_delayed_sensor(p, mu, cov, mu_n, cov_n, dt, lag, models, z, Q, mount=smr.IDENTITY_MOUNT, point=(0.0, 0.0, 0.0), rate=None,
                          latch_b=None, in_a=None, in_b=None, initialised=None, gate_chi2=-1.0):
    """The whole call.  lag [B] or a scalar, models [B] or a scalar (sensor-frame ids), z [B, 3], Q [B, 3, 3] or [3, 3], mount
    [B, 7] or [7], point [B, 3] or [3]; rate [B, 3] or None, latch_b [B, 3]: the engine's latched rotation rate (rate_source).
    -> the dict of delayed_reference.update_delayed"""
    man = p.man
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    mu_n, cov_n = np.asarray(mu_n, dtype=np.float64), np.asarray(cov_n, dtype=np.float64)
    steps, B, D = mu.shape[0], mu.shape[1], man.D
    n = steps - 1
    lag = np.broadcast_to(np.asarray(lag, dtype=np.int64), (B,))
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    z = np.asarray(z, dtype=np.float64)
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, 3, 3))
    mount = np.broadcast_to(np.asarray(mount, dtype=np.float64), (B, 7))
    point = np.broadcast_to(np.asarray(point, dtype=np.float64), (B, 3))
    live = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    w = np.zeros((B, 3))
    if p.model == "orient":
        w = rate_source(lag, steps, rate, in_b, latch_b)
    mvalid = np.isin(models, smr.ids_of(man))
    st = np.zeros(B, np.uint32)
    st = np.where(~live, on.ST_UNINITIALISED, st)
    inactive = live & ((lag < 0) | ~mvalid)
    st = np.where(inactive, on.ST_INACTIVE, st)
    old = live & ~inactive & (lag > n)
    st = np.where(old, on.ST_ERR_NEG_DT, st)
    fin = np.ones(B, bool)
    for i in np.nonzero(mvalid)[0]:
        uz, uq, um, up = smr.used_inputs(int(models[i]))
        fin[i] = (np.isfinite(z[i][uz]).all() and np.isfinite(Q[i][uq]).all() and np.isfinite(mount[i][um]).all() and
                  np.isfinite(point[i][up]).all() and (models[i] != smr.ORIENT_VELOCITY or np.isfinite(w[i]).all()))
    bad = live & ~inactive & ~old & ~fin
    st = np.where(bad, on.ST_ERR_NONFINITE_MEAS, st)
    do_u = live & ~inactive & ~old & ~bad

    o = dict(mu=mu_n.copy(), cov=cov_n.copy(), mu_out=np.full_like(mu_n, np.nan), cov_out=np.full_like(cov_n, np.nan),
             z_pred=np.full((B, 4), np.nan), S=np.full((B, 3, 3), np.nan), innov=np.full((B, 3), np.nan),
             maha=np.full(B, np.nan), loglik=np.full(B, np.nan), committed=np.zeros(B, bool))
    idx = np.nonzero(do_u)[0]
    if len(idx):
        sub = lambda x: None if x is None else (x[:, idx] if np.ndim(x) == 3 else x[idx])   # noqa: E731
        q = copy.copy(p)
        if np.ndim(q.R) == 3:
            q.R = q.R[idx]
        ms, Cs, M, good, cst = dr.backward_chain(q, mu[:, idx], cov[:, idx], mu_n[idx], cov_n[idx], dt, lag[idx], sub(in_a), sub(in_b))
        st[idx] |= cst
        for mid in np.unique(models[idx]):
            mid = int(mid)
            k = np.nonzero(models[idx] == mid)[0]
            i = idx[k]
            m = smr.meas_dim(mid)
            manz = on.VECT(m)
            _, _, um, up = smr.used_inputs(mid)
            # entries the model does not read never meet arithmetic
            mt = np.where(um, mount[i], smr.IDENTITY_MOUNT)[:, None, :]
            pt = np.where(up, point[i], 0.0)[:, None, :]
            gy = (w[i] if mid == smr.ORIENT_VELOCITY else np.zeros((len(i), 3)))[:, None, :]
            hh = lambda X: smr.h(mid, X, mt, pt, gy)   # noqa: E731
            with np.errstate(all="ignore"):
                Cs_s = np.where(good[k][:, None, None], Cs[k], np.eye(D)[None])
                u = scored_update(man, manz, ms[k], Cs_s, z[i][:, :m], hh, Q[i][:, :m, :m], p.mean_tol, p.mean_max_it, gate_chi2)
                X, _ = on.sigma_points(man, ms[k], Cs_s)
                Cxz = on.cross_cov_sigma_points(man, manz, ms[k], u.mz, X, u.Z)
                # (Sigma^s_s and S decide; the verdict of scored_update's own commit, on the PAST state, is not this call's)
                ok_s = u.ok & on.cholesky_lower(u.S)[1]
                S_s = np.where(ok_s[:, None, None], u.S, np.eye(m)[None])
                Si = np.linalg.inv(S_s)
                accept = np.ones(len(k), bool) if gate_chi2 < 0 else (u.d2 <= gate_chi2)
                U = np.linalg.solve(Cs_s, Cxz)                                   # (Sigma^s_s)^-1 C_z
                K = cov_n[i] @ np.swapaxes(M[k], 1, 2) @ U @ Si                  # Sigma_n M_s^T U S^-1
                sig2 = cov_n[i] - K @ S_s @ np.swapaxes(K, 1, 2)
                sig2 = np.tril(sig2) + np.swapaxes(np.tril(sig2, -1), 1, 2)
                okc = good[k] & ok_s & np.isfinite(sig2).all(axis=(1, 2))
                sig2s = np.where((okc & accept)[:, None, None], sig2, np.eye(D)[None])
                m2, C2, ok2 = on.apply_delta(man, mu_n[i], sig2s, np.einsum("bij,bj->bi", K, u.innov))
                loglik = -0.5 * (u.d2 + u.logdet + m * smr.LN_2PI)
            noconv = good[k] & u.ok & ((u.status & on.ST_WARN_MEAN_NOCONV) != 0)
            commit_through_history(o, st, i, okc, ok2, accept, noconv, u.mz, u.S, u.innov, u.d2, loglik, np.arange(m), np.arange(m), m2, C2)
    o["status"] = st.astype(np.uint32)
    return o


# ------------------------------------------------------------------------------------------------ a dtype per stage
@contextlib.contextmanager
def _sensor_models_in_delayed_f32(model, models, mount, point, w):
    """delayed_reference.delayed_f32 asks feature_f32.cycle_model for (m, measurement manifold, h) of every id among its rows,
    in np.unique order, and applies h to the rows of that id in their order.  While this context is open the answer is the
    sensor-frame model of that id with those rows' mounts, points and rates -- the h of feature_f32.sensor_meas: float64 in
    every mode, as the kernel evaluates the sensor models in double."""
    import feature_f32 as ff
    keep = ff.cycle_model

    def sensor_model(_, mid):
        i = np.nonzero(models == mid)[0]
        m = smr.meas_dim(mid)
        _, _, um, up = smr.used_inputs(mid)
        mt = np.where(um, mount[i], smr.IDENTITY_MOUNT)[:, None, :]
        pt = np.where(up, point[i], 0.0)[:, None, :]
        gy = (w[i] if mid == smr.ORIENT_VELOCITY else np.zeros((len(i), 3)))[:, None, :]

        def hh(X):
            one = X.ndim == 2
            return smr.h(mid, X.astype(np.float64), mt[:, 0] if one else mt, pt[:, 0] if one else pt, gy[:, 0] if one else gy).astype(X.dtype)
        return m, ff.vect(m), hh
    ff.cycle_model = sensor_model
    try:
        yield
    finally:
        ff.cycle_model = keep


def delayed_sensor_f32(p, mu, cov, mu_n, cov_n, dt, lag, models, z, Q, mount, point, w=None, in_a=None, in_b=None, prec="f32"):
    """delayed_f32 with the sensor-frame models, for rows that commit (no status handling) -> (mu [B, S], cov [B, D, D]) as an
    engine of storage precision `prec` stores them.  w [B, 3]: the rotation rate model 5 reads (rate_source)."""
    B = np.asarray(mu).shape[1]
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    mount = np.broadcast_to(np.asarray(mount, dtype=np.float64), (B, 7))
    point = np.broadcast_to(np.asarray(point, dtype=np.float64), (B, 3))
    w = np.zeros((B, 3)) if w is None else np.asarray(w, dtype=np.float64)
    with _sensor_models_in_delayed_f32(p.model, models, mount, point, w):
        return dr.delayed_f32(p, mu, cov, mu_n, cov_n, dt, lag, models, np.asarray(z, dtype=np.float64), Q, in_a, in_b, prec=prec)
