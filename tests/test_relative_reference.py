"""Pins tests/relative_reference.py, the NumPy statement of the relative-measurement update (include/ukf_batch_relative.h), on the CPU: the yardstick of tests/test_gpu_relative.py must itself be right.  The figures the tests print are
kept in profiles/relative_parity.txt."""
import numpy as np
import pytest

import delayed_reference as dr
import relative_cases as rc
import relative_reference as rr
import smoother_reference as sr
from engine_support import scaled

N, STEPS = 64, 6
_HIST = {}


def hist(spe):
    if "hot" not in _HIST:
        _HIST["hot"] = rc.cpu_history(spe, N, STEPS)
    return _HIST["hot"]


# ------------------------------------------------------------------------------------------------ 1. the linear (p, v) system
# 4 x the largest figures this reference measures over the four lags (2.22e-9 for the mean, 4.47e-12 for the covariance:
# profiles/relative_parity.txt); the mean's is the rotation variance 1e-12 of the embedding seen through R(q_s)^T (p_n - p_s)
LINEAR_MEAN_BOUND, LINEAR_COV_BOUND = 4 * 2.22e-9, 4 * 4.47e-12


@pytest.mark.parametrize("lag", [1, 2, 5, 32])
def test_linear_system_equals_the_cloned_kalman_filter(lag):
    """relative position over `lag` steps against the textbook Kalman filter that carries the clone of x_s explicitly"""
    steps, B = lag + 1, 16
    x, P, dt, acc = rc.linear_filter(steps, B)
    z_rel = x[-1, :, :3] - x[0, :, :3] + np.random.default_rng(9).uniform(-0.05, 0.05, (B, 3))
    x_in, P_in, _, _ = rc.linear_filter(steps, B, clone_at=0, z_rel=z_rel)
    mu, cov = rc.embed(x, P)
    z = np.full((B, 7), np.nan); z[:, :3] = z_rel          # the model reads its own part only
    Q = np.full((6, 6), np.nan); Q[:3, :3] = rc.R_REL
    r = rr.update_relative(rc.linear_params(), mu, cov, mu[-1], cov[-1], dt, lag, rr.POSITION, z, Q, in_a=acc)
    assert not r["status"].any() and r["committed"].all() and not r["clamped"].any()
    ex = scaled(r["mu"][:, rc.PVS], x_in[-1])
    eP = scaled(r["cov"][np.ix_(range(B), rc.PV, rc.PV)], P_in[-1])
    moved = scaled(x[-1], x_in[-1])
    print(f"RELATIVE linear lag={lag}: scaled error mean {ex:.3e} cov {eP:.3e} (the sample moves the present by {moved:.3e})")
    assert moved > 1e-4, "the increment must matter"
    assert ex <= LINEAR_MEAN_BOUND and eP <= LINEAR_COV_BOUND


# ------------------------------------------------------------------------------------------------ 2. the joint covariance, dense
@pytest.mark.parametrize("lag", [1, 3, 5])
def test_block_factor_is_the_dense_cholesky_of_the_joint_covariance(spe, onp, lag):
    """(L_n, 0; M L_n, L_e) and the 49 pairs against cholesky_lower of the explicit 24 x 24 covariance of (x_n, x_s).  Bound:
    the factorisation's backward error 24 eps, amplified by the condition of the correlation-scaled joint covariance (its own
    smallest eigenvalue, computed here from the input), with a factor 64 for the constants"""
    p, mu, cov, dt, ia = hist(spe)
    D = 12
    ms, Cs, M, good, st = dr.backward_chain(p, mu, cov, mu[-1], cov[-1], dt, np.full(N, lag), ia, None)
    assert good.all() and not st.any()
    Sn = cov[-1]
    J = np.block([[Sn, Sn @ np.swapaxes(M, 1, 2)], [M @ Sn, Cs]])
    J = np.tril(J) + np.swapaxes(np.tril(J, -1), 1, 2)
    s = np.sqrt(np.einsum("bii->bi", J))
    lam = np.linalg.eigvalsh(J / (s[:, :, None] * s[:, None, :])).min(axis=1)
    bound = 64 * 24 * np.finfo(float).eps / lam
    Ld, ok = onp.cholesky_lower(J)
    Ln, ok_n = onp.cholesky_lower(Sn)
    E = rr.sigma_e(Cs, M, Sn)
    Le, ok_e, clamped = rr.chol_clamped(E, np.einsum("bii->bi", Cs))
    assert ok.all() and ok_n.all() and ok_e.all() and not clamped.any(), "no pivot is clamped on the hot history"
    Lb = np.block([[Ln, np.zeros_like(Ln)], [M @ Ln, Le]])
    eL = (np.abs(Ld - Lb) / s[:, :, None]).max(axis=(1, 2))
    # the pairs: columns j < D of the dense factor are the first 2 D pairs, the others move the clone alone
    dn, ds = rr.pair_offsets(Ln, M @ Ln, Le)
    dn_d, ds_d = np.zeros_like(dn), np.zeros_like(ds)
    for j in range(2 * D):
        dn_d[:, 1 + 2 * j], dn_d[:, 2 + 2 * j] = Ld[:, :D, j], -Ld[:, :D, j]
        ds_d[:, 1 + 2 * j], ds_d[:, 2 + 2 * j] = Ld[:, D:, j], -Ld[:, D:, j]
    man = p.man
    Xn, Xs = man.boxplus(mu[-1][:, None, :], dn), man.boxplus(ms[:, None, :], ds)
    Xn_d, Xs_d = man.boxplus(mu[-1][:, None, :], dn_d), man.boxplus(ms[:, None, :], ds_d)
    eX = np.maximum((np.abs(man.boxminus(Xn, Xn_d)) / s[:, None, :D]).max(axis=(1, 2)),
                    (np.abs(man.boxminus(Xs, Xs_d)) / s[:, None, D:]).max(axis=(1, 2)))
    lam_e = np.linalg.eigvalsh(E / np.sqrt(np.einsum("bi,bj->bij", np.einsum("bii->bi", Cs), np.einsum("bii->bi", Cs)))).min()
    print(f"RELATIVE joint lag={lag}: factor {eL.max():.3e} pairs {eX.max():.3e} (largest share of the bound {(np.maximum(eL, eX) / bound).max():.3e}; "
          f"smallest eigenvalue of the scaled joint covariance {lam.min():.3e}, of Sigma_e scaled by Sigma^s_s {lam_e:.3e})")
    assert (eL <= bound).all() and (eX <= bound).all()
    # ... and the update made from these pairs is a valid posterior that matters
    models, z, Q = rc.increments(spe, N, mu[-1], mu[STEPS - 1 - lag])
    r = rr.update_relative(p, mu, cov, mu[-1], cov[-1], dt, lag, models, z, Q, in_a=ia)
    moved = scaled(r["mu"], mu[-1])
    ratio = np.trace(r["cov"], axis1=1, axis2=2) / np.trace(cov[-1], axis1=1, axis2=2)
    print(f"RELATIVE hot lag={lag}: the update moves the mean by {moved:.3e} scaled, trace ratio {ratio.min():.3f} ... {ratio.max():.3f}, "
          f"smallest posterior eigenvalue {np.linalg.eigvalsh(r['cov']).min():.3e}")
    assert not r["status"].any() and r["committed"].all() and moved > 1e-4
    assert (ratio < 1.0).all() and np.linalg.eigvalsh(r["cov"]).min() > 0.0


# ------------------------------------------------------------------------------------------------ 3. the clamp
def quiet_block_history(spe, onp, noise):
    """the hot history with the process noise of the angular-velocity block (tangent 9 ... 11) replaced by noise * I and its
    coupling removed: with noise = 0 the past angular velocity is determined by the present one, Sigma_e is singular there"""
    sy = spe.synth
    R = sy.pose_default_process_noise().copy()
    R[9:12, :] = 0.0
    R[:, 9:12] = 0.0
    R[9:12, 9:12] = noise * np.eye(3)
    p = sr.Params("pose", R, acc_cov=rc.ACC_COV)
    dt = np.array([dr.HOT_DT * (1.0 + 0.1 * c) for c in range(STEPS - 1)])
    mu, cov = dr.hot_initial(sy, "pose", N)
    mus, covs, ia, a = [], [], [], None
    for c in range(STEPS):
        a_, _, mid, z, Q = dr.hot_cycle_inputs(sy, "pose", N, c, mu)
        if c > 0:
            mu, cov, s1 = onp.pose_predict(mu, cov, R, a, rc.ACC_COV, dt[c - 1])
            mu, cov, s2 = onp.pose_update(mu, cov, mid, z, Q)
            assert not s1.any() and not s2.any()
        a = a_
        mus.append(mu); covs.append(cov); ia.append(a)
    return p, np.array(mus), np.array(covs), dt, np.array(ia)


CLAMP_LAG = 3   # (every step of the chain has the quiet block: the lag includes every clamped direction)


def test_zero_process_noise_is_the_limit_of_small_noise(spe, onp):
    p0, mu0, cov0, dt, ia0 = quiet_block_history(spe, onp, 0.0)
    models, z, Q = rc.increments(spe, N, mu0[-1], mu0[STEPS - 1 - CLAMP_LAG])
    r0 = rr.update_relative(p0, mu0, cov0, mu0[-1], cov0[-1], dt, CLAMP_LAG, models, z, Q, in_a=ia0)
    assert not r0["status"].any() and r0["committed"].all()
    assert (r0["clamped"] == 3).all(), "the three directions of the quiet block are clamped, no other"
    assert np.isfinite(r0["mu"]).all() and np.isfinite(r0["cov"]).all() and np.isfinite(r0["loglik"]).all()
    d = {}
    for noise in (1e-8, 1e-10, 1e-12):
        p, mu, cov, _, ia = quiet_block_history(spe, onp, noise)
        r = rr.update_relative(p, mu, cov, mu[-1], cov[-1], dt, CLAMP_LAG, models, z, Q, in_a=ia)
        assert not r["status"].any() and not r["clamped"].any()
        d[noise] = max(scaled(r["mu"], r0["mu"]), scaled(r["cov"], r0["cov"]))
        print(f"RELATIVE clamp: process noise {noise:.0e} on the quiet block is {d[noise]:.3e} scaled from zero noise")
    # the limit: the distance falls with the noise, and at 1e-12 it is inside the fp64 parity gate
    assert d[1e-12] < d[1e-10] < d[1e-8] and d[1e-12] <= 1e-9


def test_indefinite_conditional_covariance_is_refused(spe, onp):
    """Sigma_e negative beyond tau in a clamped direction: ERR_CHOLESKY, and the filter keeps every bit"""
    p0, mu0, cov0, dt, ia0 = quiet_block_history(spe, onp, 0.0)
    models, z, Q = rc.increments(spe, N, mu0[-1], mu0[STEPS - 1 - CLAMP_LAG])
    ms, Cs, M, good, st = dr.backward_chain(p0, mu0, cov0, mu0[-1], cov0[-1], dt, np.full(N, CLAMP_LAG), ia0, None)
    assert good.all() and not st.any()
    ok = rr.update_relative(p0, mu0, cov0, mu0[-1], cov0[-1], dt, CLAMP_LAG, models, z, Q, in_a=ia0, chain=(ms, Cs, M, good, st))
    assert not ok["status"].any()
    Cs2 = Cs.copy()
    hurt = np.arange(N) % 2 == 0
    Cs2[hurt, 10, 10] *= 1.0 - 1e4 * rr.TAU          # Sigma_e[10][10] = -1e4 tau a_kk: far beyond the clamp, far below any gate
    r = rr.update_relative(p0, mu0, cov0, mu0[-1], cov0[-1], dt, CLAMP_LAG, models, z, Q, in_a=ia0, chain=(ms, Cs2, M, good, st))
    assert (r["status"][hurt] == onp.ST_ERR_CHOLESKY).all() and not r["status"][~hurt].any()
    assert not r["committed"][hurt].any() and np.isnan(r["mu_out"][hurt]).all() and np.isnan(r["maha"][hurt]).all()
    assert np.array_equal(r["mu"][hurt], mu0[-1][hurt]) and np.array_equal(r["cov"][hurt], cov0[-1][hurt])
    assert np.array_equal(r["mu"][~hurt], ok["mu"][~hurt]) and np.array_equal(r["cov"][~hurt], ok["cov"][~hurt])


# ------------------------------------------------------------------------------------------------ 4. statuses
def test_statuses(spe, onp):
    p, mu, cov, dt, ia = hist(spe)
    lag = np.full(N, 2)
    models, z, Q = rc.increments(spe, N, mu[-1], mu[STEPS - 3])
    clean = rr.update_relative(p, mu, cov, mu[-1], cov[-1], dt, lag, models, z, Q, in_a=ia)
    assert not clean["status"].any()
    lag = lag.copy(); models = models.copy()
    z = np.where(np.isnan(z), rr.h_pair(mu[-1], mu[STEPS - 3]), z)   # (every part finite, so that a filter can change its model)
    lag[1], lag[2], lag[3], lag[11] = STEPS, 1000, -1, 0
    models[4] = -1; models[5] = 3
    z[6, 0] = np.nan; models[6] = rr.POSE
    z[12, 5] = np.inf; models[12] = rr.ROTATION
    z[13, 3:] = np.nan; models[13] = rr.POSITION          # the other part: not read
    QQ = np.broadcast_to(Q, (N, 6, 6)).copy()
    QQ[14, 4, 1] = np.nan; models[14] = rr.POSE          # a lower-triangle entry the model reads
    QQ[15, 1, 4] = np.nan; models[15] = rr.POSE          # the upper triangle is not read
    QQ[16, 4, 1] = np.nan; models[16] = rr.POSITION      # outside the model's rows and columns
    init = np.ones(N, bool); init[7] = False
    cov2 = cov.copy(); cov2[4, 8] = -np.eye(12); cov2[2, 9] = -np.eye(12)   # inside the chain of filter 8; below filter 9's
    mu2 = mu.copy(); mu2[3, 10, 0] = np.nan
    r = rr.update_relative(p, mu2, cov2, mu[-1], cov[-1], dt, lag, models, z, QQ, in_a=ia, initialised=init)
    st = r["status"]
    assert st[1] == onp.ST_ERR_NEG_DT and st[2] == onp.ST_ERR_NEG_DT
    assert st[3] == onp.ST_INACTIVE and st[11] == onp.ST_INACTIVE, "an increment over no steps measures nothing"
    assert st[4] == onp.ST_INACTIVE and st[5] == onp.ST_INACTIVE
    assert st[6] == onp.ST_ERR_NONFINITE_MEAS and st[12] == onp.ST_ERR_NONFINITE_MEAS and st[14] == onp.ST_ERR_NONFINITE_MEAS
    assert st[13] == 0 and st[15] == 0 and st[16] == 0, "what a model does not read may be NaN"
    assert st[7] == onp.ST_UNINITIALISED
    assert st[8] == onp.ST_ERR_CHOLESKY and st[10] == onp.ST_ERR_CHOLESKY and st[9] == 0
    quiet = [1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 14]
    assert not r["committed"][quiet].any() and np.isnan(r["mu_out"][quiet]).all() and np.isnan(r["maha"][quiet]).all()
    assert np.array_equal(r["mu"][quiet], mu[-1][quiet]) and np.array_equal(r["cov"][quiet], cov[-1][quiet])
    others = np.ones(N, bool); others[quiet + [13, 15, 16]] = False
    assert np.array_equal(r["mu"][others], clean["mu"][others]) and np.array_equal(r["cov"][others], clean["cov"][others])
    # entries outside the model's part are zero
    m1, m2 = others & (models == rr.POSITION), others & (models == rr.ROTATION)
    assert not r["z_pred"][m1, 3:].any() and not r["innov"][m1, 3:].any() and not r["S"][m1, 3:, :].any() and not r["S"][m1, :, 3:].any()
    assert not r["z_pred"][m2, :3].any() and not r["innov"][m2, :3].any() and not r["S"][m2, :3, :].any() and not r["S"][m2, :, :3].any()
    # a gated dt inside the chain passes chain and M through and leaves its code; one below the chain leaves nothing
    models, z, Q = rc.increments(spe, N, mu[-1], mu[STEPS - 3])
    dtg = dt.copy(); dtg[4] = 0.0
    g = rr.update_relative(p, mu, cov, mu[-1], cov[-1], dtg, 2, models, z, Q, in_a=ia)
    assert (g["status"] == onp.ST_SKIPPED_SMALL_DT).all() and g["committed"].all()
    dtg = dt.copy(); dtg[0] = 0.0
    g = rr.update_relative(p, mu, cov, mu[-1], cov[-1], dtg, 2, models, z, Q, in_a=ia)
    assert not g["status"].any()
    # a gate that rejects: the scores out, nothing committed
    far = z.copy(); far[:, :3] += 50.0; far[:, 3:7] = onp.quat_mul(far[:, 3:7], onp.so3_exp(np.full((N, 3), 1.0), 1.0))
    g = rr.update_relative(p, mu, cov, mu[-1], cov[-1], dt, 2, models, far, Q, in_a=ia, gate_chi2=9.0)
    assert (g["status"] == onp.ST_REJECTED_GATE).all() and not g["committed"].any() and np.isfinite(g["maha"]).all()
    assert np.isnan(g["mu_out"]).all() and np.array_equal(g["mu"], mu[-1])
    # a mean iteration that is cut short
    import copy
    q = copy.copy(p); q.mean_max_it = 1; q.mean_tol = 1e-30
    g = rr.update_relative(q, mu, cov, mu[-1], cov[-1], dt, 2, models, z, Q, in_a=ia)
    assert (g["status"] & onp.ST_WARN_MEAN_NOCONV).all()


# ------------------------------------------------------------------------------------------------ 5. the fp32 study
MIXED_LAG = 1 + np.arange(N) % 5


def test_plain_fp32_holds_the_gate(spe):
    """the all-float32 evaluation of the call beside its float64 evaluation on the GPU test's inputs: the scaled distances with
    each candidate piece in float64, and the project's 1e-4 for the evaluation with none"""
    p, mu, cov, dt, ia = hist(spe)
    models, z, Q = rc.increments(spe, N, mu[-1], mu[STEPS - 1 - MIXED_LAG, np.arange(N)])
    r = rr.update_relative(p, mu, cov, mu[-1], cov[-1], dt, MIXED_LAG, models, z, Q, in_a=ia)
    assert not r["status"].any()
    zz = np.where(np.isnan(z), 0.0, z)
    r64 = rr.relative_f32(p, mu, cov, mu[-1], cov[-1], dt, MIXED_LAG, models, zz, Q, ia, prec="f64")
    e64 = max(scaled(r64[0], r["mu"]), scaled(r64[1], r["cov"]))
    print(f"RELATIVE float64 evaluation by stages against the reference: {e64:.3e}")
    assert e64 <= 1e-12
    for wide in ((), ("sigma_e",), ("M",), ("commit",), ("M", "sigma_e", "commit")):
        r32 = rr.relative_f32(p, mu, cov, mu[-1], cov[-1], dt, MIXED_LAG, models, zz, Q, ia, prec="f32", wide=wide)
        em, ec = scaled(r32[0], r64[0]), scaled(r32[1], r64[1])
        print(f"RELATIVE float32 evaluation, float64 pieces {wide or 'none'}: mean {em:.3e} cov {ec:.3e}")
        if not wide:
            assert em <= 1e-4 and ec <= 1e-4


# ------------------------------------------------------------------------------------------------ 6. recorded: the shortcut
def test_compose_and_feed_absolute_is_overconfident(spe, onp):
    """recorded, not asserted beyond sanity: the increment composed onto the stored mean of step s and fed as an absolute pose
    of the present (an ordinary update with the increment's Q) against the cloned result"""
    p, mu, cov, dt, ia = hist(spe)
    for lag in (1, 3, 5):
        s = STEPS - 1 - lag
        _, z, Q = rc.increments(spe, N, mu[-1], mu[s])
        z = np.where(np.isnan(z), rr.RZ.boxplus(rr.h_pair(mu[-1], mu[s]), np.zeros((N, 6))), z)
        r = rr.update_relative(p, mu, cov, mu[-1], cov[-1], dt, lag, rr.POSE, z, Q, in_a=ia)
        assert not r["status"].any()
        z_abs, Q_abs = rr.compose_absolute(p, mu[s], cov[s], rr.POSE, z, Q)
        m2, C2, st = onp.ukf_update(p.man, rr.RZ, mu[-1], cov[-1], z_abs, lambda X: X[..., :7], Q_abs)
        assert not st.any()
        sd = np.sqrt(np.einsum("bii->bi", r["cov"]))
        off = (np.abs(p.man.boxminus(m2, r["mu"])) / sd).max()
        var = (np.einsum("bii->bi", C2) / np.einsum("bii->bi", r["cov"]))[:, :6]
        print(f"RELATIVE shortcut lag={lag}: compose-and-feed-absolute lands {off:.3e} posterior sigmas from the cloned result; its pose "
              f"variances are {var.min():.3f} ... {var.max():.3f} (median {np.median(var):.3f}) of the cloned ones")
        assert np.isfinite(off) and np.isfinite(var).all()
