"""NumPy float64 statement of the delayed-measurement update of include/ukf_batch.h ("late samples"): the smoother's backward
chain from the engine's present state down to the step a late sample was taken at, the cross-covariance operator M carried
along it, ukfom's measurement half on the smoothed past state and the retrodicted commit into the present.  Built on
tests/smoother_reference.py (the redone prediction and its noise, the Jr^-1 transport) and oracle.ukf_numpy.  A helper, not
collected; tests/test_delayed_reference.py pins it.

Arrays are in WINDOW order (step 0 = the oldest): mu [steps, B, S], cov [steps, B, D, D], dt [steps - 1]; step n = steps - 1
of the window arrays is never read (the engine's own state mu_n, cov_n stands there).  in_a / in_b as in smoother_reference.
`delayed_f32` is the same call with a dtype per stage (tests/feature_f32.py), the d_32 of the scaled parity."""
import numpy as np

from oracle import ukf_numpy as on
from bank_reference import jr_inv, rot_offset, hat
import smoother_reference as sr
from update_reference import commit_through_history

LN_2PI = 1.8378770664093454835606594728112
JR_SMALL_T = 0.25   # theta^2 up to which the second coefficient of Jr comes from its series (as Jr^-1's, ukf_bank.hpp)


def jr_coeffs(th):
    """(a, b) of Jr(phi) = I - a [phi]x + b [phi]x^2.  a = (1 - cos t) / t^2 = sinc(t / 2)^2 / 2: the half-angle form has no
    cancellation at any angle.  b = (t - sin t) / t^3 = (1 - sinc(t / 2) cos(t / 2)) / t^2 above JR_SMALL_T (the difference
    loses 6 eps / t^2 relative, which b [phi]x^2 turns into eps absolute); below it the series in t^2 through t^12 (the next
    term is 1.7e-19 at the edge)."""
    th = np.asarray(th)
    t = th.dtype.type if th.dtype.kind == "f" else np.float64
    h = t(0.5) * th
    sh = np.where(h == 0, t(1), np.sin(np.where(h == 0, t(1), h)) / np.where(h == 0, t(1), h))
    a = t(0.5) * sh * sh
    t2 = th * th
    small = t2 <= t(JR_SMALL_T)
    ser = t(1.0 / 1307674368000.0)
    for k in (-1.0 / 6227020800.0, 1.0 / 39916800.0, -1.0 / 362880.0, 1.0 / 5040.0, -1.0 / 120.0, 1.0 / 6.0):
        ser = ser * t2 + t(k)
    b = np.where(small, ser, (t(1) - sh * np.cos(h)) / np.where(small, t(1), t2))
    return a, b


def jr(p):
    """Jr(phi), the right Jacobian of SO(3): exp(phi + d) = exp(phi) exp(Jr(phi) d) to first order in d"""
    p = np.asarray(p)
    th = np.sqrt(np.sum(p * p, axis=-1))
    a, b = jr_coeffs(th)
    H = hat(p.astype(np.float64)).astype(p.dtype)
    return np.eye(3, dtype=p.dtype) - a[..., None, None] * H + b[..., None, None] * (H @ H)


def block_identity(D, ro, B3):
    """the D x D identity with B3 [B, 3, 3] on the SO(3) block"""
    J = np.broadcast_to(np.eye(D, dtype=B3.dtype), (B3.shape[0], D, D)).copy()
    J[:, ro:ro + 3, ro:ro + 3] = B3
    return J


def meas_model(model, mid):
    """-> (m, measurement manifold, h, is_so3) of measurement model id 0 ... 9 (include/ukf_batch.h), None if the id is not one
    of this engine's"""
    mid = int(mid)
    if model == "orient":
        if mid != on.MEAS_ORIENT_BODYVEL3:
            return None
        return 3, on.VECT(3), (lambda X: on.quat_rotate(on.quat_inverse(X[..., 0:4]), X[..., 4:7])), False
    if mid == on.MEAS_ORIENT_SO3:
        return 3, on.SO3, (lambda X: X[..., 3:7]), True
    if mid not in on._POSE_SELECT:
        return None
    idx = on._POSE_SELECT[mid]
    return len(idx), on.VECT(len(idx)), (lambda X: X[..., idx]), False


def chain_step(p, mu, cov, mu_s, cov_s, M, dt, in_a, in_b, use_J=True, use_A=True):
    """One backward step for every row: the smoother's steps 1-6 (smoother_reference.backward_step, whose chain this returns
    bit for bit) and M_c = A(delta_rot) G_c J(e_rot) M_{c+1}.  -> (mu_s_c, cov_s_c, M_c, good [B], status [B]); a gated dt
    returns the inputs and its code."""
    man = p.man
    B, D, ro = mu.shape[0], man.D, rot_offset(man)
    gate = on.gate_dt(np.full(B, float(dt)), p.min_dt, p.max_dt)
    if gate.any():
        return mu_s.copy(), cov_s.copy(), M.copy(), np.ones(B, bool), gate
    g, R = sr._process_and_noise(p, mu, dt, in_a, in_b)
    with np.errstate(all="ignore"):
        X, ok = on.sigma_points(man, mu, cov)
        Y = g(X)
        m_pred, conv = on.mean_sigma_points(man, Y, p.mean_tol, p.mean_max_it)
        Cp = on.cov_sigma_points(man, m_pred, Y) + R
        C = on.cross_cov_sigma_points(man, man, mu, m_pred, X, Y)
        _, ok_p = on.cholesky_lower(Cp)
        good = ok & ok_p
        Cp_s = np.where(good[:, None, None], Cp, np.eye(D)[None])
        G = np.swapaxes(np.linalg.solve(Cp_s, np.swapaxes(C, 1, 2)), 1, 2)
        e = man.boxminus(mu_s, m_pred)
        J = block_identity(D, ro, jr_inv(e[:, ro:ro + 3]) if use_J else np.broadcast_to(np.eye(3), (B, 3, 3)))
        St = J @ cov_s @ np.swapaxes(J, 1, 2)
        Sig = cov + G @ (St - Cp) @ np.swapaxes(G, 1, 2)
        Sig = np.tril(Sig) + np.swapaxes(np.tril(Sig, -1), 1, 2)
        fin = np.isfinite(Sig).all(axis=(1, 2))
        Sig_s = np.where((good & fin)[:, None, None], Sig, np.eye(D)[None])
        delta = np.einsum("bij,bj->bi", G, e)
        m, Cn, ok_c = on.apply_delta(man, mu, Sig_s, delta)
        A = block_identity(D, ro, jr(delta[:, ro:ro + 3]) if use_A else np.broadcast_to(np.eye(3), (B, 3, 3)))
        Mn = A @ G @ J @ M
    good = good & ok_c & fin & np.isfinite(Mn).all(axis=(1, 2))
    st = np.where(good, 0, on.ST_ERR_CHOLESKY) | np.where(conv | ~ok, 0, on.ST_WARN_MEAN_NOCONV)
    return m, Cn, Mn, good, st.astype(np.uint32)


def backward_chain(p, mu, cov, mu_n, cov_n, dt, lag, in_a=None, in_b=None, use_J=True, use_A=True):
    """The chain of every row from step n down to its own step n - lag[row] (rows with a lag outside 0 ... n stay at step n).
    -> (mu_s [B, S], cov_s [B, D, D], M [B, D, D], good [B], status [B])"""
    steps, B, D = mu.shape[0], mu.shape[1], p.man.D
    n = steps - 1
    dt = np.asarray(dt, dtype=np.float64).reshape(n)
    lag = np.asarray(lag, dtype=np.int64)
    reach = np.where((lag >= 0) & (lag <= n), lag, 0)
    ring = lambda x, c: None if x is None else (x[c] if np.ndim(x) == 3 else x)   # noqa: E731
    ms, Cs = np.array(mu_n, dtype=np.float64), np.array(cov_n, dtype=np.float64)
    M = np.broadcast_to(np.eye(D), (B, D, D)).copy()
    good, st = np.ones(B, bool), np.zeros(B, np.uint32)
    for c in range(n - 1, n - 1 - int(reach.max(initial=0)), -1):
        act = (n - reach) <= c
        m2, C2, M2, g2, s2 = chain_step(p, mu[c], cov[c], ms, Cs, M, dt[c], ring(in_a, c), ring(in_b, c), use_J, use_A)
        go = act & good & g2   # a row whose chain broke is refused: what it carries on no longer matters
        ms, Cs, M = np.where(go[:, None], m2, ms), np.where(go[:, None, None], C2, Cs), np.where(go[:, None, None], M2, M)
        good = good & (g2 | ~act)
        st = st | np.where(act, s2, 0).astype(np.uint32)
    return ms, Cs, M, good, st


def update_delayed(p, mu, cov, mu_n, cov_n, dt, lag, models, z, Q, in_a=None, in_b=None, initialised=None, gate_chi2=-1.0,
                   use_J=True, use_A=True):
    """The whole call.  lag [B] or a scalar, models [B] or a scalar, z [B, 3] (axis-angle for model 3), Q [B, 3, 3] or [3, 3].
    -> dict(mu, cov: the present state after the call; mu_out, cov_out: the corrected present state, NaN where nothing is
    committed; z_pred [B, 4], S [B, 3, 3], innov [B, 3], maha [B], loglik [B]; status [B]; committed [B])"""
    man = p.man
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    mu_n, cov_n = np.asarray(mu_n, dtype=np.float64), np.asarray(cov_n, dtype=np.float64)
    steps, B, D = mu.shape[0], mu.shape[1], man.D
    n = steps - 1
    lag = np.broadcast_to(np.asarray(lag, dtype=np.int64), (B,))
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    z = np.asarray(z, dtype=np.float64)
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, 3, 3))
    live = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    mvalid = np.array([meas_model(p.model, m) is not None for m in models])
    st = np.zeros(B, np.uint32)
    st = np.where(~live, on.ST_UNINITIALISED, st)
    inactive = live & ((lag < 0) | ~mvalid)
    st = np.where(inactive, on.ST_INACTIVE, st)
    old = live & ~inactive & (lag > n)
    st = np.where(old, on.ST_ERR_NEG_DT, st)
    mdim = np.array([meas_model(p.model, m)[0] if v else 3 for m, v in zip(models, mvalid)])
    bad = live & ~inactive & ~old & ~np.array([np.isfinite(z[i, :mdim[i]]).all() for i in range(B)])
    st = np.where(bad, on.ST_ERR_NONFINITE_MEAS, st)
    do_u = live & ~inactive & ~old & ~bad

    o = dict(mu=mu_n.copy(), cov=cov_n.copy(), mu_out=np.full_like(mu_n, np.nan), cov_out=np.full_like(cov_n, np.nan),
             z_pred=np.full((B, 4), np.nan), S=np.full((B, 3, 3), np.nan), innov=np.full((B, 3), np.nan),
             maha=np.full(B, np.nan), loglik=np.full(B, np.nan), committed=np.zeros(B, bool))
    idx = np.nonzero(do_u)[0]
    if len(idx):
        sub = lambda x: None if x is None else (x[:, idx] if np.ndim(x) == 3 else x[idx])   # noqa: E731
        import copy
        q = copy.copy(p)
        if np.ndim(q.R) == 3:
            q.R = q.R[idx]
        ms, Cs, M, good, cst = backward_chain(q, mu[:, idx], cov[:, idx], mu_n[idx], cov_n[idx], dt, lag[idx], sub(in_a), sub(in_b),
                                              use_J, use_A)
        st[idx] |= cst
        for mid in np.unique(models[idx]):
            k = np.nonzero(models[idx] == mid)[0]
            i = idx[k]
            m, manz, h, so3 = meas_model(p.model, mid)
            zz = on.so3_exp(z[i], 1.0) if so3 else z[i, :m]
            QQ = Q[i][:, :m, :m]
            with np.errstate(all="ignore"):
                Cs_s = np.where(good[k][:, None, None], Cs[k], np.eye(D)[None])
                X, ok = on.sigma_points(man, ms[k], Cs_s)
                Z = h(X)
                mz, conv = on.mean_sigma_points(manz, Z, p.mean_tol, p.mean_max_it)
                S = on.cov_sigma_points(manz, mz, Z) + QQ
                Cxz = on.cross_cov_sigma_points(man, manz, ms[k], mz, X, Z)
                _, ok_s = on.cholesky_lower(S)
                S_s = np.where(ok_s[:, None, None], S, np.eye(m)[None])
                Si = np.linalg.inv(S_s)
                nu = manz.boxminus(zz, mz)
                maha = np.einsum("bi,bij,bj->b", nu, Si, nu)
                lndet = np.log(np.linalg.det(S_s))
                accept = np.ones(len(k), bool) if gate_chi2 < 0 else (maha <= gate_chi2)
                U = np.linalg.solve(Cs_s, Cxz)                                   # (Sigma^s_s)^-1 C_z
                K = cov_n[i] @ np.swapaxes(M[k], 1, 2) @ U @ Si                  # Sigma_n M_s^T U S^-1
                sig2 = cov_n[i] - K @ S_s @ np.swapaxes(K, 1, 2)
                sig2 = np.tril(sig2) + np.swapaxes(np.tril(sig2, -1), 1, 2)
                okc = good[k] & ok & ok_s & np.isfinite(sig2).all(axis=(1, 2))
                sig2s = np.where((okc & accept)[:, None, None], sig2, np.eye(D)[None])
                m2, C2, ok2 = on.apply_delta(man, mu_n[i], sig2s, np.einsum("bij,bj->bi", K, nu))
                loglik = -0.5 * (maha + lndet + m * LN_2PI)
            commit_through_history(o, st, i, okc, ok2, accept, good[k] & ok & ~conv, mz, S, nu, maha, loglik,
                                   np.arange(mz.shape[1]), np.arange(m), m2, C2)
    o["status"] = st.astype(np.uint32)
    return o


def lag_rule(step_ts_us, sample_ts_us):
    """ukfb_delayed_lag_dev on the host: l = n - c*, c* the step nearest the sample (ties: the older step); a sample newer than
    step n gives 0; one older than step 0 by more than half of step_ts[1] - step_ts[0] gives `steps` (out of the window)"""
    ts = np.asarray(step_ts_us, dtype=np.int64)
    steps, n = len(ts), len(ts) - 1
    out = np.empty(len(sample_ts_us), np.int32)
    half0 = (ts[1] - ts[0]) if steps > 1 else 0
    for i, t in enumerate(np.asarray(sample_ts_us, dtype=np.int64)):
        if t >= ts[n]:
            out[i] = 0
        elif 2 * (ts[0] - t) > half0:
            out[i] = steps
        else:
            best = 0
            for c in range(1, steps):
                if abs(int(ts[c] - t)) < abs(int(ts[best] - t)):   # strictly nearer: ties stay with the older step
                    best = c
            out[i] = n - best
    return out


# ------------------------------------------------------------------------------------------------ test histories
# Hot histories: wide rotation spreads, large rotation rates and corrections, so that the two transports of the chain (J, A) are
# far above the parity gates (tests/test_delayed_reference.py measures by how much).
HOT_DT = 0.05
HOT = dict(rot=3.0, rate=3.0, fix=2.0, vel=1.0)   # multiples of synth's rotation sigma, rates, orientation-fix offset, velocity offset


def hot_initial(sy, model, n):
    mu, cov = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
    D = cov.shape[-1]
    ro = 3 if model == "pose" else 0
    s = np.ones(D)
    s[ro:ro + 3] = HOT['rot']                      # rotation sigma 0.05 -> 0.3 rad
    if model == "pose":
        mu = mu.copy()
        mu[:, 10:13] *= HOT['rate']                # angular velocity up to 2 rad / s
        s[9:12] = HOT['rate']                      # ... and its sigma 0.2 rad / s
    return mu, cov * s[:, None] * s[None, :]


def hot_cycle_inputs(sy, model, n, c, mu):
    """-> (a, b, meas model of the in-order cycle, z, Q): Pose alternates position fixes and orientation fixes that sit 0.2 rad
    off the estimate; OrientationState gets body velocities up to 0.5 m / s off with gyro rates up to 2 rad / s"""
    if model == "pose":
        acc, z, Q = sy.pose_cycle_inputs(n, c, mu[:, :3])
        acc[::5] = np.nan
        if c % 2 == 1:
            off = HOT['fix'] * (z - mu[:, :3])     # +-0.2 rad
            zq = on.quat_mul(mu[:, 3:7], on.so3_exp(off, 1.0))
            return acc, np.zeros((n, 3)), on.MEAS_ORIENT_SO3, on.so3_log(zq), Q * 4.0
        return acc, np.zeros((n, 3)), on.MEAS_POS3, z, Q
    gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu[:, 0:4])
    return acc, HOT['rate'] * gyro, on.MEAS_ORIENT_BODYVEL3, HOT['vel'] * z, Q


def hot_params(sy, model, acc_cov):
    if model == "pose":
        return sr.Params("pose", sy.pose_default_process_noise(), acc_cov=acc_cov)
    return sr.Params("orient", sy.orient_process_noise(), tau_g=sy.ORIENT_TAU, tau_a=sy.ORIENT_TAU,
                     earth=on.earth_rotation(sy.ORIENT_LATITUDE))


def hot_late_sample(sy, model, n, mu_s):
    """-> (models [n], z [n, 3], Q [3, 3]) of a late sample taken near the states mu_s [n, S]: sample covariance comparable to
    Sigma.  Pose cycles through its nine models, OrientationState has the one"""
    noise = sy.uniform(sy.SEED_BASE + 21, np.arange(n), [0, 1, 2], -1.0, 1.0)
    noise = np.sign(noise) * (0.04 + 0.04 * np.abs(noise))   # every component 0.8 ... 1.6 sample sigmas off: every sample matters
    if model == "pose":
        models = (np.arange(n) % 9).astype(np.int32)
        z = sy.pose_measurement_for_model(mu_s, models, noise)
    else:
        models = np.full(n, on.MEAS_ORIENT_BODYVEL3, np.int32)
        z = on.quat_rotate(on.quat_inverse(mu_s[:, 0:4]), mu_s[:, 4:7]) + noise
    return models, z, 0.05 ** 2 * np.eye(3)


# ------------------------------------------------------------------------------------------------ a dtype per stage
def delayed_f32(p, mu, cov, mu_n, cov_n, dt, lag, models, z, Q, in_a=None, in_b=None, prec="f32", wide=()):
    """The same call with the stage dtypes of tests/feature_f32.py, for rows that commit (no status handling) -> (mu [B, S],
    cov [B, D, D]) as an engine of storage P.ts stores them.  wide: the pieces done in float64 whatever prec says, any of
    "M" (the operator M and its products), "solve" (U = Sigma^-1 C_z and Y_n), "commit" (Sigma_n - Y_n Y_n^T)."""
    import feature_f32 as ff
    import study_f32_mixed as stm
    P = ff.PRECISIONS[prec]
    F64 = np.float64
    model = p.model
    man, ro, D = ff.STATE[model], ff.ROT[model], ff.STATE[model].D
    mu, cov = np.asarray(mu, dtype=F64), np.asarray(cov, dtype=F64)
    steps, B = mu.shape[0], mu.shape[1]
    n = steps - 1
    lag = np.broadcast_to(np.asarray(lag, dtype=np.int64), (B,))
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=F64), (B, 3, 3))
    dt = np.asarray(dt, dtype=F64).reshape(n)
    tM = F64 if "M" in wide else P.tl
    ring = lambda x, c: None if x is None else (x[c] if np.ndim(x) == 3 else x)   # noqa: E731
    mun, covn = np.asarray(mu_n, dtype=F64).astype(P.ts), np.asarray(cov_n, dtype=F64).astype(P.ts)
    ms, Cs = mun.astype(P.tc), covn.astype(P.tl)
    M = np.broadcast_to(np.eye(D, dtype=tM), (B, D, D)).copy()
    for c in range(n - 1, n - 1 - int(lag.max(initial=0)), -1):
        if not dt[c] > p.min_dt:
            continue
        act = (n - lag) <= c
        muc, covc = mu[c].astype(P.ts), cov[c].astype(P.ts).astype(P.tl)
        in_ac, in_bc = ring(in_a, c), ring(in_b, c)
        _, R = sr._process_and_noise(p, muc.astype(F64), dt[c], in_ac, in_bc)
        bc = lambda a, X: (a[:, None, :] if X.ndim == 3 else a).astype(X.dtype)   # noqa: E731
        if model == "pose":
            use = np.zeros(B, bool) if in_ac is None else np.isfinite(in_ac).all(axis=-1)
            acc = np.where(use[:, None], np.zeros((B, 3)) if in_ac is None else in_ac, 0.0)
            g = lambda X: stm.pose_process(X, bc(acc, X), dt[c])                     # noqa: E731
        else:
            g = lambda X: stm.orient_process(X, bc(in_ac, X), bc(in_bc, X), p.tau_g, p.earth.astype(X.dtype), dt[c])   # noqa: E731
        L = stm.chol(covc)
        X0, Xp, Xm = stm.sigma_points(man, muc, L, P)
        Y0, Yp, Ym = g(X0), g(Xp), g(Xm)
        m_pred = stm.manifold_mean(man, Y0, Yp, Ym, P)
        mm = m_pred.astype(P.tm)[:, None, :]
        dp, dm = man.minus(Yp, mm).astype(P.tl), man.minus(Ym, mm).astype(P.tl)
        d0 = man.minus(Y0.astype(P.tm), mm[:, 0]).astype(P.tl)
        Cp = 0.5 * (ff._outer_sum(dp, dp) + ff._outer_sum(dm, dm) + d0[:, :, None] * d0[:, None, :]) + R.astype(P.tl)
        cols = np.swapaxes(L, 1, 2)
        C = 0.5 * (ff._outer_sum(cols, dp) - ff._outer_sum(cols, dm))
        G = np.swapaxes(np.linalg.solve(Cp, np.swapaxes(C, 1, 2)), 1, 2)
        e = man.minus(ms.astype(P.tm), m_pred.astype(P.tm)).astype(P.tl)
        J = block_identity(D, ro, ff.jr_inv(e[:, ro:ro + 3]))
        St = J @ Cs.astype(P.tl) @ np.swapaxes(J, 1, 2)
        Sig = covc + G @ (St - Cp) @ np.swapaxes(G, 1, 2)
        Sig = np.tril(Sig) + np.swapaxes(np.tril(Sig, -1), 1, 2)
        delta = (G @ e[:, :, None])[:, :, 0]
        m2, C2 = ff.apply_delta(man, muc, Sig, delta, P)
        A = block_identity(D, ro, jr(delta[:, ro:ro + 3]))
        M2 = A.astype(tM) @ G.astype(tM) @ J.astype(tM) @ M
        ms = np.where(act[:, None], m2, ms)
        Cs = np.where(act[:, None, None], C2, Cs)
        M = np.where(act[:, None, None], M2, M)
    mu_o, cov_o = np.empty((B, man.S)), np.empty((B, D, D))
    tS = F64 if "solve" in wide else P.tl
    tC = F64 if "commit" in wide else P.tl
    for mid in np.unique(models):
        i = np.nonzero(models == mid)[0]
        m, manz, h = ff.cycle_model(model, int(mid))
        zz = stm.so3_exp(z[i].astype(P.tm)) if manz is ff.SO3 else z[i][:, :m]
        s = ff.statistics(man, manz, ms[i].astype(P.tc), Cs[i], h, Q[i][:, :m, :m], P)
        nu = ff.innovation(manz, zz.astype(P.ts), s["zbar"], P)
        Ls = stm.chol(s["S"])
        Ys = np.swapaxes(np.linalg.solve(Ls, np.swapaxes(s["Cxz"], 1, 2)), 1, 2)          # C_z Ls^-T
        y = np.linalg.solve(Ls, nu[:, :, None])
        U = np.linalg.solve(Cs[i].astype(tS), Ys.astype(tS))
        Yn = covn[i].astype(tS) @ np.swapaxes(M[i].astype(tS if tS == F64 else tM), 1, 2).astype(tS) @ U
        cov2 = covn[i].astype(tC) - Yn.astype(tC) @ np.swapaxes(Yn.astype(tC), 1, 2)
        cov2 = (0.5 * (cov2 + np.swapaxes(cov2, 1, 2))).astype(P.tl)
        m2, C2 = ff.apply_delta(man, mun[i], cov2, (Yn.astype(P.tl) @ y)[:, :, 0], P)
        mu_o[i], cov_o[i] = m2.astype(P.ts).astype(F64), C2.astype(P.ts).astype(F64)
    return mu_o, cov_o
