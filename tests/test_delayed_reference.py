"""Pins tests/delayed_reference.py, the NumPy statement of the delayed-measurement update (include/ukf_batch.h, "late
samples"), on the CPU: the yardstick of tests/test_gpu_delayed.py must itself be right.  The figures the tests print are kept in
profiles/delayed_parity.txt."""
import numpy as np
import pytest

import delayed_reference as dr
import smoother_reference as sr
from engine_support import scaled

ACC_COV = 0.01 * np.eye(3)
PV = [0, 1, 2, 6, 7, 8]          # tangent indices of (p, v) in PoseWithVelocity
PVS = [0, 1, 2, 7, 8, 9]         # ... and the stored ones


# ------------------------------------------------------------------------------------------------ the linear (p, v) system
ROT_VAR = 1e-12
Q6 = np.zeros((6, 6)); Q6[:3, :3] = 0.01 * np.eye(3); Q6[3:, 3:] = 2.0 * ACC_COV
R_POS, R_VEL = 0.05 ** 2 * np.eye(3), 0.08 ** 2 * np.eye(3)
H_POS, H_VEL = np.eye(6)[:3], np.eye(6)[3:]


def kf_update(x, P, z, H, R):
    S = H @ P @ H.T + R
    K = P @ H.T @ np.linalg.inv(S)
    return x + np.einsum("bij,bj->bi", K, z - x @ H.T), P - K @ S @ np.swapaxes(K, -1, -2)


def linear_filter(steps, B, late=(), seed=5):
    """The textbook Kalman filter of Pose's (p, v) at identity orientation, zero angular velocity, the acceleration branch
    (p' = p + dt v + dt^2 a, v' = v + dt a, the raw noise): position fixes at every step, and the samples late = [(step, z)]
    (velocity fixes) processed IN ORDER -> (x [steps, B, 6], P [steps, B, 6, 6], dt, acc)"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-5, 5, (B, 3)), rng.uniform(-1, 1, (B, 3))], axis=-1)
    G = rng.uniform(-1, 1, (B, 6, 6))
    P = 0.01 * (np.eye(6) + G @ np.swapaxes(G, -1, -2) / 6.0)
    dt = 0.02 + 0.03 * rng.uniform(0, 1, steps - 1)
    acc = rng.uniform(-0.5, 0.5, (steps, B, 3))
    zs = rng.uniform(-5, 5, (steps, B, 3))
    xs, Ps = [], []
    for c in range(steps):
        if c > 0:
            F = np.eye(6); F[:3, 3:] = dt[c - 1] * np.eye(3)
            x = x @ F.T + np.concatenate([dt[c - 1] ** 2 * acc[c - 1], dt[c - 1] * acc[c - 1]], axis=-1)
            P = F @ P @ F.T + Q6
            x, P = kf_update(x, P, zs[c], H_POS, R_POS)   # (fixes that do not depend on the state: the in-order run sees the same)
        for s, z in late:
            if s == c:
                x, P = kf_update(x, P, z, H_VEL, R_VEL)
        xs.append(x); Ps.append(P)
    return np.array(xs), np.array(Ps), dt, acc


def embed(x, P):
    """(p, v) records -> PoseWithVelocity records: identity orientation, zero angular velocity, ROT_VAR on their diagonals"""
    steps, B = x.shape[:2]
    mu = np.zeros((steps, B, 13)); mu[..., 6] = 1.0
    mu[..., PVS] = x
    cov = np.zeros((steps, B, 12, 12))
    cov[np.ix_(range(steps), range(B), PV, PV)] = P
    for k in (3, 4, 5, 9, 10, 11):
        cov[..., k, k] = ROT_VAR
    return mu, cov


def linear_params():
    return sr.Params("pose", np.diag([0.01] * 3 + [ROT_VAR] * 3 + [0.0] * 3 + [ROT_VAR] * 3), acc_cov=ACC_COV)


@pytest.mark.parametrize("lag", [1, 2, 5, 32])
def test_linear_system_equals_the_in_order_filter(onp, lag):
    """for a linear system the delayed update is exact: the bound is the one of test_smoother_reference's textbook comparison
    (1e-9 scaled at rotation variance 1e-12)"""
    steps, B = lag + 1, 16
    x, P, dt, acc = linear_filter(steps, B)
    z = x[0, :, 3:] + np.random.default_rng(9).uniform(-0.2, 0.2, (B, 3))
    x_in, P_in, _, _ = linear_filter(steps, B, late=[(0, z)])
    mu, cov = embed(x, P)
    r = dr.update_delayed(linear_params(), mu, cov, mu[-1], cov[-1], dt, lag, onp.MEAS_VEL3, z, R_VEL, in_a=acc)
    assert not r["status"].any() and r["committed"].all()
    ex = scaled(r["mu"][:, PVS], x_in[-1])
    eP = scaled(r["cov"][np.ix_(range(B), PV, PV)], P_in[-1])
    moved = scaled(x[-1], x_in[-1])
    print(f"DELAYED linear lag={lag}: scaled error mean {ex:.3e} cov {eP:.3e} (the sample moves the present by {moved:.3e})")
    assert moved > 1e-4, "the late sample must matter"
    assert ex <= 1e-9 and eP <= 1e-9


def test_two_late_samples_in_one_window_are_approximate(onp):
    """recorded, not asserted beyond sanity: the ring is not rewritten after a commit, so the second sample's chain runs over
    records that do not know the first (include/ukf_batch.h)"""
    steps, B = 6, 16
    x, P, dt, acc = linear_filter(steps, B)
    rng = np.random.default_rng(10)
    z1, z2 = x[2, :, 3:] + rng.uniform(-0.2, 0.2, (B, 3)), x[3, :, 3:] + rng.uniform(-0.2, 0.2, (B, 3))
    x_in, P_in, _, _ = linear_filter(steps, B, late=[(2, z1), (3, z2)])
    mu, cov = embed(x, P)
    p = linear_params()
    r1 = dr.update_delayed(p, mu, cov, mu[-1], cov[-1], dt, 3, onp.MEAS_VEL3, z1, R_VEL, in_a=acc)
    r2 = dr.update_delayed(p, mu, cov, r1["mu"], r1["cov"], dt, 2, onp.MEAS_VEL3, z2, R_VEL, in_a=acc)
    ex, eP = scaled(r2["mu"][:, PVS], x_in[-1]), scaled(r2["cov"][np.ix_(range(B), PV, PV)], P_in[-1])
    e0 = scaled(x[-1], x_in[-1])
    print(f"DELAYED two late samples, ring not rewritten: scaled error mean {ex:.3e} cov {eP:.3e} (both dropped: {e0:.3e})")
    assert not r2["status"].any() and np.isfinite(ex) and np.isfinite(eP)


# ------------------------------------------------------------------------------------------------ the nonlinear histories
def cpu_history(spe, onp, model, n, steps, late_at=None, late=None, inputs=None):
    """the recording of tests/test_gpu_delayed.py with the NumPy oracle as the filter; `inputs` replays a recording's inputs
    (they depend on the state they were drawn at), `late` = (models, z, Q) is processed in order at step late_at"""
    sy = spe.synth
    p = dr.hot_params(sy, model, ACC_COV)
    dt = np.array([dr.HOT_DT * (1.0 + 0.1 * c) for c in range(steps - 1)])
    mu, cov = dr.hot_initial(sy, model, n)
    mus, covs, ia, ib, rec = [], [], [], [], []
    a = b = None
    for c in range(steps):
        a_, b_, mid, z, Q = dr.hot_cycle_inputs(sy, model, n, c, mu) if inputs is None else inputs[c]
        rec.append((a_, b_, mid, z, Q))
        if c > 0:
            if model == "pose":
                mu, cov, s1 = onp.pose_predict(mu, cov, p.R, a, ACC_COV, dt[c - 1])
                mu, cov, s2 = onp.pose_update(mu, cov, mid, z, Q)
            else:
                mu, cov, s1 = onp.orient_predict(mu, cov, p.R, a, b, p.tau_g, p.tau_a, p.earth, dt[c - 1])
                mu, cov, s2 = onp.orient_update(mu, cov, z, Q)
            assert not s1.any() and not s2.any()
        if late_at == c:
            models, zl, Ql = late
            QQ = np.broadcast_to(Ql, (n, 3, 3))
            mu, cov, s3 = onp.pose_update_mixed(mu, cov, models, zl, QQ) if model == "pose" else onp.orient_update(mu, cov, zl, QQ)
            assert not s3.any()
        a, b = a_, b_
        mus.append(mu); covs.append(cov); ia.append(a); ib.append(b)
    return p, np.array(mus), np.array(covs), dt, np.array(ia), np.array(ib), rec


N, STEPS = 256, 6
_HIST = {}


def hist(spe, onp, model):
    if model not in _HIST:
        _HIST[model] = cpu_history(spe, onp, model, N, STEPS)
    return _HIST[model]


def mixed_call(spe, onp, model, **kw):
    p, mu, cov, dt, ia, ib, _ = hist(spe, onp, model)
    lag = np.arange(N) % STEPS
    models, z, Q = dr.hot_late_sample(spe.synth, model, N, mu[STEPS - 1 - lag, np.arange(N)])
    return dr.update_delayed(p, mu, cov, mu[-1], cov[-1], dt, lag, models, z, Q, ia, ib, **kw), (lag, models, z, Q)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_chain_is_the_smoothers_and_lag_zero_is_the_update(spe, onp, model):
    p, mu, cov, dt, ia, ib, _ = hist(spe, onp, model)
    ms, Cs, M, good, st = dr.backward_chain(p, mu, cov, mu[-1], cov[-1], dt, np.full(N, STEPS - 1), ia, ib)
    mu_s, cov_s, st_s, _ = sr.smooth(p, mu, cov, dt, in_a=ia, in_b=ib)
    assert good.all() and not st.any() and not st_s.any()
    assert np.array_equal(ms, mu_s[0]) and np.array_equal(Cs, cov_s[0]), "the chain is the smoother's, bit for bit"
    # lag 0: the ordinary update of the present state
    models, z, Q = dr.hot_late_sample(spe.synth, model, N, mu[-1])
    r = dr.update_delayed(p, mu, cov, mu[-1], cov[-1], dt, 0, models, z, Q, ia, ib)
    QQ = np.broadcast_to(Q, (N, 3, 3))
    m0, C0, s0 = onp.pose_update_mixed(mu[-1], cov[-1], models, z, QQ) if model == "pose" else onp.orient_update(mu[-1], cov[-1], z, QQ)
    assert not r["status"].any() and not s0.any()
    em, ec = scaled(r["mu"], m0), scaled(r["cov"], C0)
    print(f"DELAYED {model} lag 0 against the ordinary update: {em:.3e} {ec:.3e}")
    # (Sigma Sigma^-1 C_z in place of C_z: rounding times the condition of Sigma, nothing else)
    assert em <= 1e-10 and ec <= 1e-10


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_transports_are_not_cosmetic(spe, onp, model):
    """A = I or J = I must move the result by at least 1e-5 scaled -- four orders above the fp64 gate of 1e-9 and a tenth of the
    fp32 gate, measured here at 1e-3 and more: otherwise the GPU parity test could not see a kernel that leaves a transport
    out"""
    r, _ = mixed_call(spe, onp, model)
    assert not r["status"].any()
    for name, kw in (("J = I", dict(use_J=False)), ("A = I", dict(use_A=False))):
        q, _ = mixed_call(spe, onp, model, **kw)
        d = max(scaled(q["mu"], r["mu"]), scaled(q["cov"], r["cov"]))
        print(f"DELAYED {model}: {name} moves the result by {d:.3e} scaled")
        assert d >= 1e-5, (name, d)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_in_order_comparison(spe, onp, model):
    """whitened distance (by the in-order covariance) of the delayed result from the in-order result, against the same distance
    of the state that dropped the sample: smaller for every filter at every lag"""
    p, mu, cov, dt, ia, ib, rec = hist(spe, onp, model)
    ratios = []
    for lag in range(1, STEPS):
        s = STEPS - 1 - lag
        models, z, Q = dr.hot_late_sample(spe.synth, model, N, mu[s])
        r = dr.update_delayed(p, mu, cov, mu[-1], cov[-1], dt, lag, models, z, Q, ia, ib)
        assert not r["status"].any()
        _, mu2, cov2, *_ = cpu_history(spe, onp, model, N, STEPS, late_at=s, late=(models, z, Q), inputs=rec)
        Li = np.linalg.cholesky(cov2[-1])
        white = lambda m: np.linalg.norm(np.linalg.solve(Li, p.man.boxminus(m, mu2[-1])[:, :, None])[:, :, 0], axis=1)   # noqa: E731
        d_del, d_drop = white(r["mu"]), white(mu[-1])
        assert (d_del < d_drop).all(), (lag, float((d_del / d_drop).max()))
        ratios.append(d_del / d_drop)
    ratios = np.concatenate(ratios)
    print(f"DELAYED {model} in-order comparison: delayed / dropped median {np.median(ratios):.3e} max {ratios.max():.3e}")


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_plain_fp32_holds_the_gate(spe, onp, model):
    """the all-float32 evaluation of the call against its float64 evaluation on these inputs: no piece needs fp64 to hold 1e-4"""
    p, mu, cov, dt, ia, ib, _ = hist(spe, onp, model)
    r, (lag, models, z, Q) = mixed_call(spe, onp, model)
    r64 = dr.delayed_f32(p, mu, cov, mu[-1], cov[-1], dt, lag, models, z, Q, ia, ib, prec="f64")
    assert scaled(r64[0], r["mu"]) <= 1e-12 and scaled(r64[1], r["cov"]) <= 1e-12
    for wide in ((), ("M",), ("solve",), ("commit",), ("M", "solve", "commit")):
        r32 = dr.delayed_f32(p, mu, cov, mu[-1], cov[-1], dt, lag, models, z, Q, ia, ib, prec="f32", wide=wide)
        em, ec = scaled(r32[0], r64[0]), scaled(r32[1], r64[1])
        print(f"DELAYED {model} float32 evaluation, float64 pieces {wide or 'none'}: mean {em:.3e} cov {ec:.3e}")
        if not wide:
            assert em <= 1e-4 / 7.0 and ec <= 1e-4 / 7.0   # the gate with feature_scaled_parity's margin M_FEAT to spare


def test_statuses(spe, onp):
    p, mu, cov, dt, ia, ib, _ = hist(spe, onp, "pose")
    lag = np.full(N, 2)
    models, z, Q = dr.hot_late_sample(spe.synth, "pose", N, mu[STEPS - 3])
    lag[1], lag[2], lag[3] = STEPS, 1000, -1
    models[4] = -1; models[5] = 9
    z = z.copy(); z[6, 0] = np.nan
    init = np.ones(N, bool); init[7] = False
    cov2 = cov.copy(); cov2[4, 8] = -np.eye(12); cov2[2, 9] = -np.eye(12)   # inside the chain of filter 8; below filter 9's
    mu2 = mu.copy(); mu2[3, 10, 0] = np.nan
    dtg = dt.copy()
    r = dr.update_delayed(p, mu2, cov2, mu[-1], cov[-1], dtg, lag, models, z, Q, ia, ib, initialised=init)
    clean = dr.update_delayed(p, mu, cov, mu[-1], cov[-1], dt, np.full(N, 2), dr.hot_late_sample(spe.synth, "pose", N, mu[STEPS - 3])[0],
                              dr.hot_late_sample(spe.synth, "pose", N, mu[STEPS - 3])[1], Q, ia, ib)
    st = r["status"]
    assert st[1] == onp.ST_ERR_NEG_DT and st[2] == onp.ST_ERR_NEG_DT
    assert st[3] == onp.ST_INACTIVE and st[4] == onp.ST_INACTIVE and st[5] == onp.ST_INACTIVE
    assert st[6] == onp.ST_ERR_NONFINITE_MEAS and st[7] == onp.ST_UNINITIALISED
    assert st[8] == onp.ST_ERR_CHOLESKY and st[10] == onp.ST_ERR_CHOLESKY and st[9] == 0
    quiet = [1, 2, 3, 4, 5, 6, 7, 8, 10]
    assert not r["committed"][quiet].any() and np.isnan(r["mu_out"][quiet]).all() and np.isnan(r["maha"][quiet]).all()
    assert np.array_equal(r["mu"][quiet], mu[-1][quiet]) and np.array_equal(r["cov"][quiet], cov[-1][quiet])
    others = np.ones(N, bool); others[quiet] = False
    assert np.array_equal(r["mu"][others], clean["mu"][others]) and np.array_equal(r["cov"][others], clean["cov"][others])
    # a gated dt inside the chain passes chain and M through and leaves its code; one below the chain leaves nothing
    dtg[4] = 0.0
    zp = mu[-1][:, :3] + 0.01
    g = dr.update_delayed(p, mu, cov, mu[-1], cov[-1], dtg, 2, 0, zp, Q, ia, ib)
    assert (g["status"] == onp.ST_SKIPPED_SMALL_DT).all() and g["committed"].all()
    dtg = dt.copy(); dtg[0] = 0.0
    g = dr.update_delayed(p, mu, cov, mu[-1], cov[-1], dtg, 2, 0, zp, Q, ia, ib)
    assert not g["status"].any()
    # a gate that rejects: statistics out, nothing committed
    g = dr.update_delayed(p, mu, cov, mu[-1], cov[-1], dt, 2, 0, mu[-1][:, :3] + 50.0, Q, ia, ib, gate_chi2=9.0)
    assert (g["status"] == onp.ST_REJECTED_GATE).all() and not g["committed"].any() and np.isfinite(g["maha"]).all()
    assert np.isnan(g["mu_out"]).all() and np.array_equal(g["mu"], mu[-1])


def test_lag_rule():
    ts = np.array([1000, 2000, 3100, 4000, 5000], dtype=np.int64)
    t = np.array([5000, 9000, 4999, 4500, 4501, 3550, 1000, 600, 500, 499, -7000, 2550, 1500], dtype=np.int64)
    #            now  newer  ~4    tie->3 ->4   tie->2 0     0    0(edge) out  out    tie->1 tie->0
    assert list(dr.lag_rule(ts, t)) == [0, 0, 0, 1, 0, 2, 4, 4, 4, 5, 5, 3, 4]


# ------------------------------------------------------------------------------------------------ Jr against 40 digits
mp = pytest.importorskip("mpmath")


def jr_mp(phi):
    mp.mp.dps = 40
    p = [mp.mpf(float(x)) for x in phi]
    th = mp.sqrt(sum(x * x for x in p))
    H = mp.matrix([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
    if th == 0:
        return mp.eye(3)
    return mp.eye(3) - ((1 - mp.cos(th)) / th ** 2) * H + ((th - mp.sin(th)) / th ** 3) * (H * H)


def test_jr_against_mpmath_at_branch_edges():
    rng = np.random.default_rng(4)
    edge = np.sqrt(dr.JR_SMALL_T)   # the series of the second coefficient ends at theta^2 = 0.25
    thetas = [0.0, 1e-300, 1e-12, 1e-6, 1e-3, 1e-2, 0.3, np.nextafter(edge, 0), edge, np.nextafter(edge, 1), 0.5 + 1e-9, 1.0, 2.5,
              np.pi - 1e-9, np.pi, 3.5, 6.0]
    worst = 0.0
    for th in thetas:
        for _ in range(4):
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            phi = th * d
            got, ref = dr.jr(phi), jr_mp(phi)
            err = max(abs(mp.mpf(float(got[i, j])) - ref[i, j]) for i in range(3) for j in range(3))
            worst = max(worst, float(err))
            assert err <= 8 * 2.0 ** -52 * (1.0 + th * th), (th, float(err))   # a few roundings per coefficient, times [phi]x, [phi]x^2
    print(f"DELAYED Jr against mpmath at 40 digits: largest absolute error {worst:.3e}")
    # Jr is the inverse of the Jr^-1 the chain already uses
    for th in (1e-3, 0.3, 2.5, 3.0, np.pi - 1e-3, np.pi - 1e-6, np.nextafter(np.pi, 0), np.pi):
        phi = th * np.array([0.6, -0.48, 0.64])
        assert np.abs(dr.jr(phi) @ dr.jr_inv(phi) - np.eye(3)).max() <= 1e-14
