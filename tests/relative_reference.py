"""NumPy float64 statement of the relative-measurement update of include/ukf_batch_relative.h: an increment
(R(q_s)^T (p_n - p_s), q_s^-1 q_n) between step s = n - lag of the history and the present, as ukfom's update on the pair
(x_n, x_s) -- the state augmented by a clone -- with only the present state kept.  Built on delayed_reference.backward_chain
(the smoothed past state and the regression M_s of x_s on x_n) and oracle.ukf_numpy.  A helper, not collected;
tests/test_relative_reference.py pins it.

Arrays are in WINDOW order as in delayed_reference.  `relative_f32` is the same call with a dtype per stage
(tests/feature_f32.py), the d_32 of the scaled parity."""
import copy

import numpy as np

from oracle import ukf_numpy as on
import delayed_reference as dr
import smoother_reference as sr
from update_reference import commit_through_history

LN_2PI = dr.LN_2PI
TAU = 64.0 * np.finfo(np.float64).eps          # the clamp of the factorisation of Sigma_e, in units of its diagonal
POSE, POSITION, ROTATION = 0, 1, 2
RZ = on._Compound([("vec", 0, 0, 3), ("so3", 3, 3, 3)])                         # R^3 x SO(3): dp, then dq as x y z w


def meas_manifold(mid):
    """-> (measurement manifold, stored indices of z, tangent rows) of model `mid`, None if there is no such model"""
    mid = int(mid)
    if mid == POSE:
        return RZ, np.arange(7), np.arange(6)
    if mid == POSITION:
        return on.VECT(3), np.arange(3), np.arange(3)
    if mid == ROTATION:
        return on.SO3, np.arange(3, 7), np.arange(3, 6)
    return None


def h_pair(Xn, Xs):
    """(R(q_s)^T (p_n - p_s), q_s^-1 q_n) -> [..., 7]; the quaternions are taken as given: q^-1 = conj(q) / |q|^2"""
    qi = on.quat_inverse(Xs[..., 3:7])
    return np.concatenate([on.quat_rotate(qi, Xn[..., 0:3] - Xs[..., 0:3]), on.quat_mul(qi, Xn[..., 3:7])], axis=-1)


def chol_clamped(A, scale, tau=TAU):
    """The clamped factorisation of a positive SEMIdefinite matrix (lower triangle): with x_k the pivot after its subtractions
    and a_kk = scale[k], x_k > tau a_kk is an ordinary column, |x_k| <= tau a_kk a zero column, x_k < -tau a_kk (or a NaN)
    fails.  scale [B, D]: the diagonal of the matrix A was formed from by subtraction (Sigma^s_s for Sigma_e): in a direction
    the present determines, A's own diagonal entry is the rounding error of that subtraction, of either sign, and measures
    nothing.  -> (L [B, D, D], ok [B], clamped [B, D])"""
    A = np.asarray(A)
    scale = np.asarray(scale, dtype=A.dtype)
    t = A.dtype.type
    B, D, _ = A.shape
    L = np.zeros_like(A)
    ok = np.ones(B, bool)
    clamped = np.zeros((B, D), bool)
    with np.errstate(all="ignore"):
        for k in range(D):
            x = A[:, k, k].copy()
            for j in range(k):
                x = x - L[:, k, j] * L[:, k, j]
            lim = t(tau) * scale[:, k]
            pos = (x > lim) & np.isfinite(x)
            zero = ~pos & (np.abs(x) <= lim)
            ok &= pos | zero
            clamped[:, k] = zero
            d = np.sqrt(np.where(pos, x, t(1)))
            L[:, k, k] = np.where(pos, d, t(0))
            for i in range(k + 1, D):
                a = A[:, i, k].copy()
                for j in range(k):
                    a = a - L[:, i, j] * L[:, k, j]
                L[:, i, k] = np.where(pos, a / d, t(0))
    return L, ok, clamped


def sigma_e(cov_s, M, cov_n):
    """Sigma_e = Sigma^s_s - M Sigma_n M^T, the lower triangle mirrored"""
    E = cov_s - M @ cov_n @ np.swapaxes(M, 1, 2)
    return np.tril(E) + np.swapaxes(np.tril(E, -1), 1, 2)


def pair_offsets(Ln, MLn, Le):
    """tangent offsets of the 4 D + 1 pairs: (0, 0); for j < D (+-L_n col j, +-(M L_n) col j); then (0, +-L_e col j)
    -> (dn [B, 4 D + 1, D], ds [B, 4 D + 1, D])"""
    B, D, _ = Ln.shape
    dn, ds = np.zeros((B, 4 * D + 1, D), Ln.dtype), np.zeros((B, 4 * D + 1, D), Ln.dtype)
    for j in range(D):
        dn[:, 1 + 2 * j], dn[:, 2 + 2 * j] = Ln[:, :, j], -Ln[:, :, j]
        ds[:, 1 + 2 * j], ds[:, 2 + 2 * j] = MLn[:, :, j], -MLn[:, :, j]
        ds[:, 2 * D + 1 + 2 * j], ds[:, 2 * D + 2 + 2 * j] = Le[:, :, j], -Le[:, :, j]
    return dn, ds


def update_relative(p, mu, cov, mu_n, cov_n, dt, lag, models, z, Q, in_a=None, in_b=None, initialised=None, gate_chi2=-1.0,
                    tau=TAU, chain=None):
    """The whole call.  lag [B] or a scalar, models [B] or a scalar, z [B, 7], Q [B, 6, 6] or [6, 6] (its lower triangle is read).
    chain: (mu_s, cov_s, M, good, status) in place of the backward chain (tests that shape Sigma_e by hand).
    -> dict(mu, cov: the present state after the call; mu_out, cov_out: NaN where nothing is committed; z_pred [B, 7],
    S [B, 6, 6], innov [B, 6] (zero outside the model's part), maha [B], loglik [B]; status [B]; committed [B]; clamped [B]:
    the zero columns of L_e)"""
    assert p.model == "pose"
    man = p.man
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    mu_n, cov_n = np.asarray(mu_n, dtype=np.float64), np.asarray(cov_n, dtype=np.float64)
    steps, B, D = mu.shape[0], mu.shape[1], man.D
    n = steps - 1
    lag = np.broadcast_to(np.asarray(lag, dtype=np.int64), (B,))
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    z = np.asarray(z, dtype=np.float64)
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, 6, 6))
    Q = np.tril(Q) + np.swapaxes(np.tril(Q, -1), 1, 2)
    live = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    mvalid = np.array([meas_manifold(m) is not None for m in models])
    st = np.zeros(B, np.uint32)
    st = np.where(~live, on.ST_UNINITIALISED, st)
    inactive = live & ((lag <= 0) | ~mvalid)
    st = np.where(inactive, on.ST_INACTIVE, st)
    old = live & ~inactive & (lag > n)
    st = np.where(old, on.ST_ERR_NEG_DT, st)

    def reads_finite(i):
        _, si, ti = meas_manifold(models[i])
        return np.isfinite(z[i, si]).all() and np.isfinite(Q[i][np.ix_(ti, ti)]).all()
    bad = live & ~inactive & ~old & ~np.array([reads_finite(i) if mvalid[i] else True for i in range(B)])
    st = np.where(bad, on.ST_ERR_NONFINITE_MEAS, st)
    do_u = live & ~inactive & ~old & ~bad

    o = dict(mu=mu_n.copy(), cov=cov_n.copy(), mu_out=np.full_like(mu_n, np.nan), cov_out=np.full_like(cov_n, np.nan),
             z_pred=np.full((B, 7), np.nan), S=np.full((B, 6, 6), np.nan), innov=np.full((B, 6), np.nan),
             maha=np.full(B, np.nan), loglik=np.full(B, np.nan), committed=np.zeros(B, bool), clamped=np.zeros(B, np.int64))
    idx = np.nonzero(do_u)[0]
    if len(idx):
        sub = lambda x: None if x is None else (x[:, idx] if np.ndim(x) == 3 else x[idx])   # noqa: E731
        q = copy.copy(p)
        if np.ndim(q.R) == 3:
            q.R = q.R[idx]
        if chain is None:
            ms, Cs, M, good, cst = dr.backward_chain(q, mu[:, idx], cov[:, idx], mu_n[idx], cov_n[idx], dt, lag[idx], sub(in_a), sub(in_b))
        else:
            ms, Cs, M, good, cst = (x[idx] for x in chain)
        st[idx] |= cst
        for mid in np.unique(models[idx]):
            k = np.nonzero(models[idx] == mid)[0]
            i = idx[k]
            manz, si, ti = meas_manifold(mid)
            m = len(ti)
            with np.errstate(all="ignore"):
                Ln, ok_n = on.cholesky_lower(cov_n[i])
                E = sigma_e(Cs[k], M[k], cov_n[i])
                Le, ok_e, clamped = chol_clamped(E, np.einsum("bii->bi", Cs[k]), tau)
                dn, ds = pair_offsets(Ln, M[k] @ Ln, Le)
                Xn, Xs = man.boxplus(mu_n[i][:, None, :], dn), man.boxplus(ms[k][:, None, :], ds)
                Z = h_pair(Xn, Xs)[..., si]
                mz, conv = on.mean_sigma_points(manz, Z, p.mean_tol, p.mean_max_it)
                S = on.cov_sigma_points(manz, mz, Z) + Q[i][:, ti[:, None], ti[None, :]]
                dz = manz.boxminus(Z, mz[:, None, :])
                W = 0.5 * (dz[:, 1:2 * D + 1:2] - dz[:, 2:2 * D + 2:2])            # [B, D, m], the first 2 D points only
                Cn = np.einsum("bij,bjm->bim", Ln, W)
                Ls, ok_s = on.cholesky_lower(S)
                Ls_s = np.where(ok_s[:, None, None], Ls, np.eye(m)[None])
                Yn = np.swapaxes(np.linalg.solve(Ls_s, np.swapaxes(Cn, 1, 2)), 1, 2)   # C_n Ls^-T
                nu = manz.boxminus(z[i][:, si], mz)
                y = np.linalg.solve(Ls_s, nu[:, :, None])[:, :, 0]
                maha = np.sum(y * y, axis=-1)
                lndet = 2.0 * np.sum(np.log(np.einsum("bii->bi", Ls_s)), axis=-1)
                accept = np.ones(len(k), bool) if gate_chi2 < 0 else (maha <= gate_chi2)
                sig2 = cov_n[i] - Yn @ np.swapaxes(Yn, 1, 2)
                sig2 = np.tril(sig2) + np.swapaxes(np.tril(sig2, -1), 1, 2)
                okc = good[k] & ok_n & ok_e & ok_s & np.isfinite(sig2).all(axis=(1, 2))
                sig2s = np.where((okc & accept)[:, None, None], sig2, np.eye(D)[None])
                m2, C2, ok2 = on.apply_delta(man, mu_n[i], sig2s, np.einsum("bim,bm->bi", Yn, y))
                loglik = -0.5 * (maha + lndet + m * LN_2PI)
            commit_through_history(o, st, i, okc, ok2, accept, good[k] & ok_n & ok_e & ~conv, mz, S, nu, maha, loglik, si, ti,
                                   m2, C2)
            o["clamped"][i] = clamped.sum(axis=1)
    o["status"] = st.astype(np.uint32)
    return o


def compose_absolute(p, mu_s, cov_s, models, z, Q):
    """The shortcut the call replaces, for POSE increments: the increment composed onto the stored mean of step s as an absolute
    pose of the present, z_abs = (p_s + R(q_s) dp, q_s dq), with the increment's Q rotated into the measurement's frame and
    nothing of Sigma_s in it -> (z_abs [B, 7], Q_abs [B, 6, 6])"""
    qs = mu_s[:, 3:7]
    z_abs = np.concatenate([mu_s[:, 0:3] + on.quat_rotate(qs, z[:, 0:3]), on.quat_mul(qs, z[:, 3:7])], axis=-1)
    R = on.quat_to_matrix(qs)
    A = np.zeros((len(mu_s), 6, 6))
    A[:, :3, :3] = R
    A[:, 3:, 3:] = np.eye(3)
    return z_abs, A @ np.broadcast_to(Q, (len(mu_s), 6, 6)) @ np.swapaxes(A, 1, 2)


# ------------------------------------------------------------------------------------------------ a dtype per stage
def _chain_f32(p, mu, cov, mun, covn, dt, lag, in_a, P, tM):
    """the chain of delayed_reference.delayed_f32 (Pose), statement for statement -> (mu_s in tc, cov_s in tl, M in tM)"""
    import feature_f32 as ff
    import study_f32_mixed as stm
    F64 = np.float64
    man, ro, D = ff.STATE["pose"], ff.ROT["pose"], ff.STATE["pose"].D
    steps, B = mu.shape[0], mu.shape[1]
    n = steps - 1
    ring = lambda x, c: None if x is None else (x[c] if np.ndim(x) == 3 else x)   # noqa: E731
    ms, Cs = mun.astype(P.tc), covn.astype(P.tl)
    M = np.broadcast_to(np.eye(D, dtype=tM), (B, D, D)).copy()
    for c in range(n - 1, n - 1 - int(lag.max(initial=0)), -1):
        if not dt[c] > p.min_dt:
            continue
        act = (n - lag) <= c
        muc, covc = mu[c].astype(P.ts), cov[c].astype(P.ts).astype(P.tl)
        in_ac = ring(in_a, c)
        _, R = sr._process_and_noise(p, muc.astype(F64), dt[c], in_ac, None)
        bc = lambda a, X: (a[:, None, :] if X.ndim == 3 else a).astype(X.dtype)   # noqa: E731
        use = np.zeros(B, bool) if in_ac is None else np.isfinite(in_ac).all(axis=-1)
        acc = np.where(use[:, None], np.zeros((B, 3)) if in_ac is None else in_ac, 0.0)
        g = lambda X: stm.pose_process(X, bc(acc, X), dt[c])                     # noqa: E731
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
        J = dr.block_identity(D, ro, ff.jr_inv(e[:, ro:ro + 3]))
        St = J @ Cs.astype(P.tl) @ np.swapaxes(J, 1, 2)
        Sig = covc + G @ (St - Cp) @ np.swapaxes(G, 1, 2)
        Sig = np.tril(Sig) + np.swapaxes(np.tril(Sig, -1), 1, 2)
        delta = (G @ e[:, :, None])[:, :, 0]
        m2, C2 = ff.apply_delta(man, muc, Sig, delta, P)
        A = dr.block_identity(D, ro, dr.jr(delta[:, ro:ro + 3]))
        M2 = A.astype(tM) @ G.astype(tM) @ J.astype(tM) @ M
        ms = np.where(act[:, None], m2, ms)
        Cs = np.where(act[:, None, None], C2, Cs)
        M = np.where(act[:, None, None], M2, M)
    return ms, Cs, M


def _h_pair_t(Xn, Xs):
    import study_f32_mixed as stm
    qi = stm.qinv(Xs[..., 3:7])
    return np.concatenate([stm.qrot(qi, Xn[..., 0:3] - Xs[..., 0:3]), stm.qmul(qi, Xn[..., 3:7])], axis=-1)


def relative_f32(p, mu, cov, mu_n, cov_n, dt, lag, models, z, Q, in_a=None, prec="f32", wide=()):
    """The same call with the stage dtypes of tests/feature_f32.py, for rows that commit (no status handling) -> (mu [B, S],
    cov [B, D, D]) as an engine of storage P.ts stores them.  wide: the pieces done in float64 whatever prec says, any of
    "M" (the operator M and its products), "sigma_e" (Sigma^s_s - M Sigma_n M^T and its clamped factorisation), "commit"
    (Sigma_n - Y_n Y_n^T)."""
    import feature_f32 as ff
    import study_f32_mixed as stm
    P = ff.PRECISIONS[prec]
    F64 = np.float64
    man, D = ff.STATE["pose"], ff.STATE["pose"].D
    manrz = ff.Fields([("vec", 0, 0, 3), ("so3", 3, 3, 3)])
    mu, cov = np.asarray(mu, dtype=F64), np.asarray(cov, dtype=F64)
    steps, B = mu.shape[0], mu.shape[1]
    lag = np.broadcast_to(np.asarray(lag, dtype=np.int64), (B,))
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=F64), (B, 6, 6))
    Q = np.tril(Q) + np.swapaxes(np.tril(Q, -1), 1, 2)
    dt = np.asarray(dt, dtype=F64).reshape(steps - 1)
    tM = F64 if "M" in wide else P.tl
    tE = F64 if "sigma_e" in wide else P.tl
    tC = F64 if "commit" in wide else P.tl
    mun, covn = np.asarray(mu_n, dtype=F64).astype(P.ts), np.asarray(cov_n, dtype=F64).astype(P.ts)
    ms, Cs, M = _chain_f32(p, mu, cov, mun, covn, dt, lag, in_a, P, tM)
    mu_o, cov_o = np.empty((B, man.S)), np.empty((B, D, D))
    sub = {POSE: manrz, POSITION: ff.vect(3), ROTATION: ff.SO3}
    for mid in np.unique(models):
        i = np.nonzero(models == mid)[0]
        _, si, ti = meas_manifold(mid)
        manz = sub[int(mid)]
        Sn = covn[i].astype(P.tl)
        Ln = stm.chol(Sn)
        E = Cs[i].astype(tE) - M[i].astype(tE) @ Sn.astype(tE) @ np.swapaxes(M[i].astype(tE), 1, 2)
        E = np.tril(E) + np.swapaxes(np.tril(E, -1), 1, 2)
        Le, ok_e, _ = chol_clamped(E, np.einsum("bii->bi", Cs[i]).astype(tE), 64.0 * np.finfo(tE).eps)
        assert ok_e.all()
        dn, ds = pair_offsets(Ln, (M[i].astype(tM) @ Ln.astype(tM)).astype(P.tl), Le.astype(P.tl))
        Xn = man.plus(np.broadcast_to(mun[i].astype(P.tm)[:, None, :], (len(i), 4 * D + 1, man.S)).copy(), dn.astype(P.tm))
        Xs = man.plus(np.broadcast_to(ms[i].astype(P.tm)[:, None, :], (len(i), 4 * D + 1, man.S)).copy(), ds.astype(P.tm))
        Z = _h_pair_t(Xn, Xs)[..., si]
        ref = Z[:, 0].astype(P.tc)
        active = np.ones(len(i), bool)
        for _ in range(100):
            d = manz.minus(Z, ref.astype(P.tm)[:, None, :]).sum(1) / P.tm(4 * D + 1)
            ref = np.where(active[:, None], manz.plus(ref, d.astype(P.tc)), ref)
            active = active & (np.sqrt((d.astype(F64) ** 2).sum(-1)) > stm.MEAN_TOL)
            if not active.any():
                break
        dz = manz.minus(Z, ref.astype(P.tm)[:, None, :]).astype(P.tl)
        S = 0.5 * ff._outer_sum(dz, dz) + Q[i][:, ti[:, None], ti[None, :]].astype(P.tl)
        W = 0.5 * (dz[:, 1:2 * D + 1:2] - dz[:, 2:2 * D + 2:2])
        Cn = np.einsum("bij,bjm->bim", Ln, W)
        Ls = stm.chol(S)
        Yn = np.swapaxes(np.linalg.solve(Ls, np.swapaxes(Cn, 1, 2)), 1, 2)
        zz = z[i][:, si].astype(P.ts)
        nu = manz.minus(zz.astype(P.tm), ref.astype(P.tm)).astype(P.tl)
        y = np.linalg.solve(Ls, nu[:, :, None])
        cov2 = Sn.astype(tC) - Yn.astype(tC) @ np.swapaxes(Yn.astype(tC), 1, 2)
        cov2 = (np.tril(cov2) + np.swapaxes(np.tril(cov2, -1), 1, 2)).astype(P.tl)
        m2, C2 = ff.apply_delta(man, mun[i], cov2, (Yn @ y)[:, :, 0], P)
        mu_o[i], cov_o[i] = m2.astype(P.ts).astype(F64), C2.astype(P.ts).astype(F64)
    return mu_o, cov_o
