"""NumPy float64 statement of the probabilistic data association update of include/ukf_batch_pda.h, made of the oracle's pieces:
update_reference.scored_update (the sigma points' images, z-bar, S and the verdicts on Sigma and S), on.cross_cov_sigma_points
(C), the association weights by a log-sum-exp, the combination in the TEXTBOOK form -- K = C S^-1,
Sigma~ = beta_0 Sigma + (1 - beta_0) (Sigma - K S K^T) + K (sum beta_k nu_k nu_k^T - nu-bar nu-bar^T) K^T, delta = K nu-bar --
and on.apply_delta.  That form is deliberately not the whitened form of the header (Sigma - Y M Y^T with y = Ls^-1 nu), which
combine_whitened states for tests/test_pda_reference.py to hold the two to each other.  The weights and the combination take
a dtype (float32: the bound of a plain fp32 engine, tests/pda_f32.py).  A helper, not collected;
tests/test_pda_reference.py pins it.

z [K, B, 3]; point [3] / [B, 3]: shared-h mode, one hypothesis per filter."""
import collections

import numpy as np

import associate_reference as ar
import sensor_meas_reference as sr
from oracle import ukf_numpy as on
from update_reference import scored_update

Rule = collections.namedtuple("Rule", "p_detect p_gate_m1 p_gate_m3 clutter_m1 clutter_m3")
FAILED = ar.FAILED
GATE = 16.0
P_DETECT = 0.9
# P(chi^2_m <= 16): m = 1: erf(sqrt(8)); m = 3: erf(sqrt(8)) - sqrt(2 / pi) 4 exp(-8)
P_GATE_M1 = 0.99993665751633376
P_GATE_M3 = 0.99886601665624511
# Chosen once for constructed_pda's batches (both engines, Q = 0.05^2 I), from beta_0 / (1 - beta_0) = lambda (1 - P_D P_G)
# sqrt(det 2 pi S) / (P_D sum_G exp(-r^2 / 2)) = 1 at a rough size of S in these batches (m = 1: S ~ 0.003 ... 0.01; m = 3:
# det S ~ 1e-8 ... 1e-6), before any result existed, and kept as they came out.  The
# share of the filters with a non-empty G that get 0.01 < beta_0 < 0.99 (tests/test_pda_reference.py prints and asserts >= 1/2;
# 140 filters on the CPU): PoseWithVelocity 0.80 (K = 1), 0.81 (K = 4), 0.84 (K = 32); OrientationState 0.75, 0.76, 0.93.  On
# the device tests' 1 022 filters as downloaded: 0.82 and 1.00 (K = 4; profiles/pda_parity.txt).
CLUTTER_M1 = 2.0
CLUTTER_M3 = 300.0
RULE = Rule(P_DETECT, P_GATE_M1, P_GATE_M3, CLUTTER_M1, CLUTTER_M3)


def kernel_dim(man, models):
    """m as the kernel takes it: the model's, 3 for an id this engine does not have (such a row rides along as a 3-vector)"""
    return np.array([sr.meas_dim(int(i)) if int(i) in sr.ids_of(man) else 3 for i in models])


def log_terms(rule, m):
    """-> (a_0 [B] = ln lambda_m + ln(1 - P_D P_G,m), ln P_D) in float64, as the host forms them"""
    m = np.asarray(m)
    lam = np.where(m == 1, rule.clutter_m1, rule.clutter_m3)
    pg = np.where(m == 1, rule.p_gate_m1, rule.p_gate_m3)
    return np.log(lam) + np.log1p(-rule.p_detect * pg), float(np.log(rule.p_detect))


def weights(loglik, inside, a0, ln_pd, dtype=np.float64):
    """loglik [K, B], inside [K, B] (the set G), a0 [B] -> (beta [K, B]: 0 outside G, beta0 [B]) by a log-sum-exp over {0} and G"""
    t = dtype
    a = np.where(inside, t(ln_pd) + np.where(inside, loglik, 0.0).astype(t), t(-np.inf)).astype(t)
    a0 = np.asarray(a0).astype(t)
    top = np.maximum(a0, a.max(axis=0))
    with np.errstate(under="ignore"):
        total = np.exp(a0 - top) + np.exp(a - top[None]).sum(axis=0, dtype=t)
        A = (top + np.log(total)).astype(t)
        return np.exp(a - A[None]).astype(t), np.exp(a0 - A).astype(t)


def combine_textbook(cov, Kg, S, nu, beta, beta0, dtype=np.float64):
    """cov [B, D, D], Kg = C S^-1 [B, D, m], S [B, m, m], nu [K, B, m], beta [K, B] (0 outside G), beta0 [B] ->
    (Sigma~ [B, D, D], delta [B, D], nu-bar [B, m]) in `dtype`"""
    t = dtype
    cov, Kg, S, nu, beta, beta0 = (np.asarray(x).astype(t) for x in (cov, Kg, S, nu, beta, beta0))
    KT = np.swapaxes(Kg, 1, 2)
    nub = np.einsum("kb,kbi->bi", beta, nu)
    spread = np.einsum("kb,kbi,kbj->bij", beta, nu, nu) - nub[:, :, None] * nub[:, None, :]
    Pc = cov - Kg @ S @ KT
    cov2 = beta0[:, None, None] * cov + (t(1) - beta0)[:, None, None] * Pc + Kg @ spread @ KT
    return cov2.astype(t), np.einsum("bij,bj->bi", Kg, nub).astype(t), nub.astype(t)


def combine_whitened(cov, C, S, nu, beta, beta0):
    """the header's form: Ls = chol(S), Y = C Ls^-T, y_k = Ls^-1 nu_k, M = (1 - beta_0) I - (sum beta y y^T - y-bar y-bar^T),
    Sigma~ = Sigma - Y M Y^T, delta = Y y-bar -> (Sigma~, delta, M)"""
    Ls = np.linalg.cholesky(S)
    Li = np.linalg.inv(Ls)
    Y = C @ np.swapaxes(Li, 1, 2)
    y = np.einsum("bij,kbj->kbi", Li, nu)
    yb = np.einsum("kb,kbi->bi", beta, y)
    Py = np.einsum("kb,kbi,kbj->bij", beta, y, y) - yb[:, :, None] * yb[:, None, :]
    M = (1.0 - beta0)[:, None, None] * np.eye(S.shape[1]) - Py
    return cov - Y @ M @ np.swapaxes(Y, 1, 2), np.einsum("bij,bj->bi", Y, yb), M


def update_pda(man, mu, cov, models, z, Q, mount, point, gyro=None, rule=RULE, gate_chi2=-1.0, initialised=None, commit=True,
               tol=on.MEAN_TOL, max_it=on.MEAN_MAX_IT, dtype=np.float64):
    """-> dict(mu, cov, z_pred [B, 3], S [B, 3, 3], innov [K, B, 3], maha, loglik, beta [K, B], beta0 [B], innov_comb [B, 3],
    best, n_gated [B], status [B])"""
    z = np.asarray(z, dtype=np.float64)
    K, B = z.shape[0], z.shape[1]
    D = man.D
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, 3, 3))
    mount = np.broadcast_to(np.asarray(mount, dtype=np.float64), (B, 7))
    point = np.broadcast_to(np.asarray(point, dtype=np.float64), (B, 3))
    gyro = np.zeros((B, 3)) if gyro is None else np.asarray(gyro, dtype=np.float64)
    init = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    valid = np.isin(models, sr.ids_of(man))
    mk = kernel_dim(man, models)
    lead = np.arange(3)[None, :] < mk[:, None]                                   # [B, 3]: the first m entries
    nanf = lambda *s: np.full(s, np.nan)   # noqa: E731
    o = {"mu": mu.copy(), "cov": cov.copy(), "z_pred": nanf(B, 3), "S": nanf(B, 3, 3), "innov": nanf(K, B, 3), "maha": nanf(K, B),
         "loglik": nanf(K, B), "beta": nanf(K, B), "beta0": nanf(B), "innov_comb": nanf(B, 3)}
    o["innov"][:, ~lead] = 0.0            # padding is 0 whatever becomes of the filter
    o["innov_comb"][~lead] = 0.0
    best, n_gated = np.full(B, -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.uint32)
    status[~init] = on.ST_UNINITIALISED
    status[init & ~valid] = on.ST_INACTIVE
    for mid in np.unique(models[init & valid]):
        mid = int(mid)
        m = sr.meas_dim(mid)
        idx = np.nonzero(init & valid & (models == mid))[0]
        _, uq, um, up = sr.used_inputs(mid)
        fin = (np.isfinite(Q[idx][:, uq]).all(axis=1) & np.isfinite(mount[idx][:, um]).all(axis=1) & np.isfinite(point[idx][:, up]).all(axis=1))
        present = np.isfinite(z[:, idx, :m]).all(axis=2)                          # [K, n]
        go = fin & present.any(axis=0)
        status[idx[~go]] = on.ST_ERR_NONFINITE_MEAS
        idx, present = idx[go], present[:, go]
        if idx.size == 0:
            continue
        n = idx.size
        manz = on.VECT(m)
        mt = np.where(um, mount[idx], sr.IDENTITY_MOUNT)[:, None, :]
        pt = np.where(up, point[idx], 0.0)[:, None, :]
        gy = gyro[idx][:, None, :]
        hh = lambda X: sr.h(mid, X, mt, pt, gy)   # noqa: E731
        zz = np.where(present[:, :, None], z[:, idx, :m], 0.0)                    # an absent candidate: neutral values
        z_any = zz[np.argmax(present, axis=0), np.arange(n)]                     # a present candidate: scored_update wants a z
        # ---- 1. z-bar, S, C and the verdicts on Sigma and S: gate 0, so that no Sigma~ is judged here
        u = scored_update(man, manz, mu[idx], cov[idx], z_any, hh, Q[idx][:, :m, :m], tol, max_it, 0.0)
        X, _ = on.sigma_points(man, mu[idx], cov[idx])
        C = on.cross_cov_sigma_points(man, manz, mu[idx], u.mz, X, u.Z)
        eye = np.eye(m)
        S = np.where(u.scored[:, None, None], u.S, eye)
        Si = np.linalg.inv(S)
        Kg = C @ Si
        # ---- 2, 3. the scores and the gate
        nu = zz - u.mz[None]
        with np.errstate(over="ignore", invalid="ignore"):
            d2 = np.einsum("kbi,bij,kbj->kb", nu, Si, nu)
        loglik = -0.5 * (d2 + u.logdet[None] + m * sr.LN_2PI)
        scored = u.scored[None] & present
        finite = scored & np.isfinite(d2)
        inside = finite & ((gate_chi2 < 0) | (np.where(finite, d2, np.inf) <= gate_chi2))
        ng = inside.sum(axis=0)
        accept = ng > 0
        # ---- 4. the weights; 5, 6. the combination; 7. applyDelta
        a0, ln_pd = log_terms(rule, np.full(n, m))
        beta, beta0 = weights(loglik, inside, a0, ln_pd, dtype)
        cov2, delta, nub = combine_textbook(cov[idx], Kg, S, np.where(inside[:, :, None], nu, 0.0), beta, beta0, dtype)
        cov2 = np.where((u.scored & accept)[:, None, None], cov2.astype(np.float64), np.eye(D))
        m2, C2, ok2 = on.apply_delta(man, mu[idx], cov2, np.where(accept[:, None], delta.astype(np.float64), 0.0))
        okc = u.scored & (ok2 | ~accept)
        st = np.where(okc, 0, on.ST_ERR_CHOLESKY).astype(np.uint32)
        st |= np.where(u.ok & ((u.status & on.ST_WARN_MEAN_NOCONV) != 0), on.ST_WARN_MEAN_NOCONV, 0).astype(np.uint32)
        st |= np.where(okc & finite.any(axis=0) & ~accept, on.ST_REJECTED_GATE, 0).astype(np.uint32)
        status[idx] = st
        # ---- the outputs of the filters that are not refused
        s_ = idx[okc]
        sc = scored[:, okc]
        o["z_pred"][s_] = 0.0
        o["z_pred"][s_, :m] = u.mz[okc]
        o["S"][s_] = 0.0
        o["S"][s_[:, None, None], np.arange(m)[None, :, None], np.arange(m)[None, None, :]] = u.S[okc]
        for k in range(K):
            o["innov"][k][s_, :m] = np.where(sc[k][:, None], nu[k][okc], np.nan)
            o["maha"][k][s_] = np.where(sc[k], d2[k][okc], np.nan)
            o["loglik"][k][s_] = np.where(sc[k], loglik[k][okc], np.nan)
            o["beta"][k][s_] = np.where(finite[k][okc], np.where(inside[k][okc], beta[k][okc].astype(np.float64), 0.0), np.nan)
        o["beta0"][s_] = beta0[okc].astype(np.float64)
        o["innov_comb"][s_, :m] = nub[okc].astype(np.float64)
        b, _ = ar.pick_best(np.where(scored, d2, np.nan), gate_chi2)
        best[s_], n_gated[s_] = b[okc], ng[okc]
        wrote = okc & accept
        if commit:
            o["mu"][idx[wrote]], o["cov"][idx[wrote]] = m2[wrote], C2[wrote]
    o["best"], o["n_gated"], o["status"] = best, n_gated, status
    return o


# ---------------------------------------------------------------------------------------------------- the constructed inputs
RADII_K4 = (1.0, 2.0, 3.0, 5.0)
RADII_OUT = (5.0, 6.0, 7.0, 8.0)


def radii(K):
    """Mahalanobis radii of the K candidates: K = 4: three inside the gate of 16 and one outside; else 0.5 + 0.3 k, spread
    across the gate (K = 32: up to 9.8); K = 1: one candidate at radius 1"""
    return np.array(RADII_K4 if K == 4 else [0.5 + 0.3 * k for k in range(K)]) if K > 1 else np.array([1.0])


def constructed_pda(man, mu, cov, models, z_true, Q, mount, point, gyro, K, dtype=np.float64, seed=23, all_outside=True):
    """-> (z [K, B, 3] as the engine stores them, radius [K, B]): candidate k of filter i is z-bar + r Ls u with S = Ls Ls^T
    the filter's own innovation covariance, u a random unit vector of the measurement space and r = radii(K)[(k + i) % K]: the
    prescribed radii, rotated by i % K.  all_outside and K = 4: every 7th filter gets the radii 5, 6, 7, 8 instead, all of them
    outside the gate of 16.  Filters without an S (no model, uninitialised) get z_true in every slot.  Whether rounding to
    `dtype` left every d^2 clear of the gate is for the caller to assert (conditions)."""
    B = mu.shape[0]
    rng = np.random.default_rng(seed)
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    m = kernel_dim(man, models)
    raw = sr.update_sensor(man, mu, cov, models, z_true, Q, mount, point, gyro, gate_chi2=0.0)
    has = ~np.isnan(raw["S"]).any(axis=(1, 2))
    S = np.where(has[:, None, None], raw["S"], np.eye(3))
    S = S + np.eye(3) * (np.arange(3)[None, :] >= m[:, None])[:, :, None]                # identity beyond m, where S is padded with 0
    Ls, _ = on.cholesky_lower(S)
    zbar = np.where(has[:, None], raw["z_pred"], z_true)
    base = radii(K)
    r = base[(np.arange(K)[:, None] + np.arange(B)[None, :]) % K]
    if all_outside and K == 4:
        out = np.arange(B) % 7 == 6
        r[:, out] = np.array(RADII_OUT)[(np.arange(K)[:, None] + np.arange(B)[None, out]) % K]
    u = rng.standard_normal((K, B, 3)) * (np.arange(3)[None, None, :] < m[None, :, None])
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    z = zbar[None] + np.where(has, r, 0.0)[:, :, None] * np.einsum("bij,kbj->kbi", Ls, u)
    return np.asarray(z, dtype=np.float64).astype(dtype).astype(np.float64), r


def conditions(ref, gate=GATE, clear=0.05):
    """The conditions of the constructed inputs, on the reference's own numbers -> the share of the filters with a non-empty G
    whose beta_0 lies in (0.01, 0.99).  Asserts that every d^2 is at least 5 % clear of the gate."""
    d2 = ref["maha"][np.isfinite(ref["maha"])]
    assert (np.abs(d2 - gate) >= clear * gate).all(), float(np.abs(d2 - gate).min())
    some = (ref["n_gated"] > 0) & ((ref["status"] & FAILED) == 0)
    b0 = ref["beta0"][some]
    return float(((b0 > 0.01) & (b0 < 0.99)).mean())
