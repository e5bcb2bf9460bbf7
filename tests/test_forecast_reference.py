"""Pins tests/forecast_reference.py, the NumPy statement of the forecast (include/ukf_batch.h, "forecast"), on the CPU: the
yardstick of tests/test_gpu_forecast.py must itself be right."""
import numpy as np
import pytest

import forecast_reference as fr
import smoother_reference as sr

ACC_COV = 0.01 * np.eye(3)
H = 5
DT = np.array([0.01, 0.013, 0.02, 0.007, 0.011])


def case(spe, onp, model, n, per_filter_noise=False, cycles=2):
    """synth's initial state after `cycles` oracle cycles (full covariances) -> (params, mu, cov, in_a [H, n, 3], in_b)"""
    sy = spe.synth
    mu, cov = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
    R = sy.pose_default_process_noise() if model == "pose" else sy.orient_process_noise()
    earth = onp.earth_rotation(sy.ORIENT_LATITUDE)
    for c in range(cycles):
        if model == "pose":
            acc, z, Q = sy.pose_cycle_inputs(n, c, mu[:, :3])
            mu, cov, s1 = onp.pose_predict(mu, cov, R, acc, ACC_COV, 0.01)
            mu, cov, s2 = onp.pose_update(mu, cov, onp.MEAS_POS3, z, Q)
        else:
            gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu[:, 0:4])
            mu, cov, s1 = onp.orient_predict(mu, cov, R, acc, gyro, sy.ORIENT_TAU, sy.ORIENT_TAU, earth, 0.01)
            mu, cov, s2 = onp.orient_update(mu, cov, z, Q)
        assert not s1.any() and not s2.any()
    ia, ib = [], []
    for c in range(H):
        if model == "pose":
            acc, _, _ = sy.pose_cycle_inputs(n, cycles + c, mu[:, :3])
            acc[::5] = np.nan   # the constant-velocity branch
            ia.append(acc); ib.append(np.zeros((n, 3)))
        else:
            gyro, acc, _, _ = sy.orient_cycle_inputs(n, cycles + c, mu[:, 0:4])
            ia.append(acc); ib.append(gyro)
    if per_filter_noise:
        R = (1.0 + np.arange(n) / n + 0.5 * (np.arange(n) % 3 == 0))[:, None, None] * R[None]
    if model == "pose":
        p = sr.Params("pose", R, acc_cov=ACC_COV)
    else:
        p = sr.Params("orient", R, tau_g=sy.ORIENT_TAU, tau_a=sy.ORIENT_TAU, earth=earth)
    return p, mu, cov, np.array(ia), np.array(ib)


def single(onp, p, mu, cov, dt, a, b):
    """one prediction by the oracle's own entry points"""
    if p.model == "pose":
        return onp.pose_predict(mu, cov, p.R, a, p.acc_cov, dt)
    return onp.orient_predict(mu, cov, p.R, a, b, p.tau_g, p.tau_a, p.earth, dt)


@pytest.mark.parametrize("per_filter_noise", [False, True])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_steps_are_the_oracles_predictions_bit_for_bit(spe, onp, model, per_filter_noise):
    """one step = pose_predict / orient_predict (both Pose branches: every fifth filter is on a NaN acceleration row); H steps
    = H single steps"""
    p, mu, cov, ia, ib = case(spe, onp, model, 37, per_filter_noise)
    if model == "pose":
        assert np.isnan(ia[0][::5]).all() and np.isfinite(ia[0][1::5]).all()
    m1, c1, st, sts = fr.forecast(p, mu, cov, dt=DT[:1], in_a=ia[:1], in_b=ib[:1])
    m, C, s = single(onp, p, mu, cov, DT[0], ia[0], ib[0])
    assert np.array_equal(m1[0], m) and np.array_equal(c1[0], C) and np.array_equal(st, s) and not s.any()
    mh, ch, st, sts = fr.forecast(p, mu, cov, dt=DT, in_a=ia, in_b=ib)
    assert mh.shape == (H,) + mu.shape and ch.shape == (H,) + cov.shape and sts.shape == (H, 37) and not st.any()
    m, C = mu, cov
    for c in range(H):
        m, C, s = single(onp, p, m, C, DT[c], ia[c], ib[c])
        assert np.array_equal(mh[c], m) and np.array_equal(ch[c], C) and not s.any(), c
    # latched inputs [B, 3] serve every step
    ml, cl, _, _ = fr.forecast(p, mu, cov, dt=DT[:2], in_a=ia[0], in_b=ib[0])
    m, C, _ = single(onp, p, mh[0], ch[0], DT[1], ia[0], ib[0])
    assert np.array_equal(ml[0], mh[0]) and np.array_equal(ml[1], m) and np.array_equal(cl[1], C)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_timestamp_form_is_the_chain_of_gate_timestamps(spe, onp, model):
    """a null last time (SKIPPED_FIRST_TS, the shadow time becomes the stamp), a repeated stamp (SKIPPED_SMALL_DT: the record
    before it, the shadow time stays) and a stamp that goes backwards (ERR_NEG_DT)"""
    n = 12
    p, mu, cov, ia, ib = case(spe, onp, model, n)
    last0 = 1_000_000 + 1000 * np.arange(n, dtype=np.int64)   # every filter its own
    last0[3] = 0                                              # null
    last0[4] = 1_020_000                                      # = ts_us[0]
    last0[5] = 1_500_000                                      # beyond every stamp
    ts = np.array([1_020_000, 1_031_000, 1_031_000, 1_025_000, 1_047_000], dtype=np.int64)
    mh, ch, st, sts = fr.forecast(p, mu, cov, ts_us=ts, last_us=last0, in_a=ia, in_b=ib)
    m, C, last = mu.copy(), cov.copy(), last0.copy()
    for c in range(H):
        new_last, dt, gate = onp.gate_timestamps(np.full(n, ts[c]), last, p.min_dt, p.max_dt)
        for i in range(n):
            if gate[i] == 0:
                mi, Ci, si = single(onp, p, m[i:i + 1], C[i:i + 1], float(dt[i]), ia[c][i:i + 1], ib[c][i:i + 1])
                m[i], C[i] = mi[0], Ci[0]
                assert si[0] == 0
        assert np.array_equal(sts[c], gate), c
        assert np.array_equal(mh[c], m) and np.array_equal(ch[c], C), c
        last = new_last
    assert sts[0, 3] == onp.ST_SKIPPED_FIRST_TS and np.array_equal(mh[0, 3], mu[3]) and sts[1, 3] == 0
    assert sts[0, 4] == onp.ST_SKIPPED_SMALL_DT and np.array_equal(ch[0, 4], cov[4])
    assert (sts[2, :3] == onp.ST_SKIPPED_SMALL_DT).all() and np.array_equal(mh[2], mh[1]) and np.array_equal(ch[2], ch[1])
    assert (sts[3, :3] == onp.ST_ERR_NEG_DT).all() and np.array_equal(mh[3], mh[2])
    # the shadow time did not advance over the repeated and the backward stamp: the last step spans 1 031 000 -> 1 047 000
    assert (sts[4, :3] == 0).all()
    m4, _, _ = single(onp, p, mh[3][:3], ch[3][:3], 0.016, ia[4][:3], ib[4][:3])
    assert np.array_equal(mh[4][:3], m4)
    assert (sts[:, 5] == onp.ST_ERR_NEG_DT).all() and np.array_equal(mh[:, 5], np.broadcast_to(mu[5], (H, mu.shape[1])))
    assert st[5] == onp.ST_ERR_NEG_DT and st[0] == (onp.ST_SKIPPED_SMALL_DT | onp.ST_ERR_NEG_DT)


def test_gating_failure_and_uninitialised(spe, onp):
    p, mu, cov, ia, ib = case(spe, onp, "pose", 8)
    dt = DT.copy()
    dt[2] = 0.0
    cov = cov.copy()
    cov[6] = -np.eye(12)
    live = np.ones(8, bool)
    live[1] = False
    mh, ch, st, sts = fr.forecast(p, mu, cov, dt=dt, in_a=ia, initialised=live)
    assert np.array_equal(mh[2, 0], mh[1, 0]) and np.array_equal(ch[2, 0], ch[1, 0])
    assert st[0] == onp.ST_SKIPPED_SMALL_DT and st[1] == onp.ST_UNINITIALISED
    assert st[6] == (onp.ST_ERR_CHOLESKY | onp.ST_SKIPPED_SMALL_DT)
    assert all(np.array_equal(mh[c, 6], mu[6]) and np.array_equal(ch[c, 6], cov[6]) for c in range(H))
    assert np.isnan(mh[:, 1]).all() and np.isnan(ch[:, 1]).all()
    with pytest.raises(AssertionError):
        fr.forecast(p, mu, cov, dt=dt, ts_us=np.arange(5), last_us=0)


def test_closed_form_constant_velocity(onp):
    """Pose, constant-velocity branch (NaN acceleration), zero angular velocity.  on.pose_process then reads
    p' = p + dt R(q) v, q' = q (+) 0 = q, v' = v: linear in (p, v) for a fixed q, and the unscented transform is exact for a
    linear map.  After H steps of total time T: p = p0 + T R(q) v0, v = v0, and with F_c = [[I, dt_c R(q)], [0, I]],
    P <- F_c P F_c^T + dt_c Q, Q the (p, v) blocks of the noise (the position block is isotropic, so its rotation by R(q)
    leaves it as it is).  The set-up is linear only up to the spread of the rotation (variance 1e-12 on the orientation and on
    the angular velocity, no noise on either): it bends R(q) v at second order, O(variance) = 1e-12 relative, three orders
    below the bound."""
    rng = np.random.default_rng(11)
    B, rot_var = 16, 1e-12
    mu = np.zeros((B, 13))
    q = rng.normal(size=(B, 4))
    mu[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    mu[:, 0:3] = rng.uniform(-5, 5, (B, 3)); mu[:, 7:10] = rng.uniform(-1, 1, (B, 3))
    G = rng.uniform(-1, 1, (B, 6, 6))
    P6 = 0.01 * (np.eye(6) + G @ np.swapaxes(G, -1, -2) / 6.0)
    pv = [0, 1, 2, 6, 7, 8]
    cov = np.zeros((B, 12, 12))
    cov[np.ix_(range(B), pv, pv)] = P6
    for k in (3, 4, 5, 9, 10, 11):
        cov[:, k, k] = rot_var
    Rn = np.diag([0.01] * 3 + [0.0] * 3 + [0.002] * 3 + [0.0] * 3)
    p = sr.Params("pose", Rn, acc_cov=ACC_COV)
    mh, ch, st, _ = fr.forecast(p, mu, cov, dt=DT, in_a=np.full((B, 3), np.nan))
    assert not st.any()
    rot = onp.quat_to_matrix(mu[:, 3:7])
    x, P = mu[:, [0, 1, 2, 7, 8, 9]].copy(), P6.copy()
    Q6 = np.diag([0.01] * 3 + [0.002] * 3)
    scaled = lambda a, b: float(np.max(np.abs(a - b) / (1.0 + np.abs(b))))   # noqa: E731
    for c in range(H):
        F = np.broadcast_to(np.eye(6), (B, 6, 6)).copy()
        F[:, :3, 3:] = DT[c] * rot
        x = np.einsum("bij,bj->bi", F, x)
        P = F @ P @ np.swapaxes(F, 1, 2) + DT[c] * Q6
        ex = scaled(mh[c][:, [0, 1, 2, 7, 8, 9]], x)
        eP = scaled(ch[c][np.ix_(range(B), pv, pv)], P)
        print(f"closed form, step {c}: scaled errors mean {ex:.3e} cov {eP:.3e}")
        assert ex <= 1e-9 and eP <= 1e-9, (c, ex, eP)
    T = DT.sum()
    assert scaled(mh[-1][:, 0:3], mu[:, 0:3] + T * np.einsum("bij,bj->bi", rot, mu[:, 7:10])) <= 1e-9
    assert scaled(mh[-1][:, 3:7], mu[:, 3:7]) <= 1e-9 and scaled(mh[-1][:, 10:13], 0.0 * mu[:, 10:13]) <= 1e-9


def test_pose_variances_do_not_decrease(spe, onp):
    """Pose from a diagonal start covariance under positive definite noise, both branches: nothing in the Pose process model
    contracts (velocity and angular velocity are carried over, position and orientation integrate them), the cross-covariances
    the integration builds from a diagonal start are those of a sum with its own summand, and every step adds noise with a
    positive diagonal.  (OrientationState is left out on purpose: its bias states decay by 1 - dt / tau.)"""
    sy = spe.synth
    n = 40
    mu, cov = sy.pose_initial(n)
    cov = np.array([np.diag(np.diag(c)) for c in cov])
    acc, _, _ = sy.pose_cycle_inputs(n, 0, mu[:, :3])
    acc[::5] = np.nan
    R = sy.pose_default_process_noise()
    assert np.linalg.eigvalsh(R).min() > 0
    p = sr.Params("pose", R, acc_cov=ACC_COV)
    _, ch, st, _ = fr.forecast(p, mu, cov, dt=np.full(8, 0.05), in_a=acc)
    assert not st.any()
    d = np.einsum("cbii->cbi", np.concatenate([cov[None], ch]))
    assert (np.diff(d, axis=0) > 0).all()
    assert np.linalg.eigvalsh(ch).min() > 0


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_float32_evaluation(spe, onp, model):
    """prec="f32": float32 in every stage, so it differs from the float64 reference -- by rounding, not by algorithm -- and its
    records are float32 values; a gated step repeats the record before it"""
    p, mu, cov, ia, ib = case(spe, onp, model, 24)
    m64, c64, _, _ = fr.forecast(p, mu, cov, dt=DT, in_a=ia, in_b=ib)
    dt = DT.copy()
    m32, c32, st, _ = fr.forecast(p, mu, cov, dt=dt, in_a=ia, in_b=ib, prec="f32")
    assert not st.any()
    assert np.array_equal(m32, m32.astype(np.float32).astype(np.float64)) and np.array_equal(c32, c32.astype(np.float32))
    em = np.max(np.abs(m32 - m64) / (1.0 + np.abs(m64)))
    ec = np.max(np.abs(c32 - c64) / (1.0 + np.abs(c64)))
    print(f"{model}: float32 evaluation against float64 over {H} steps: mean {em:.3e} cov {ec:.3e}")
    assert 0.0 < em <= 1e-4 and 0.0 < ec <= 1e-4   # the project's fp32 parity bound holds for a correct fp32 evaluation
    dt[1] = 0.0
    g32, h32, st, _ = fr.forecast(p, mu, cov, dt=dt, in_a=ia, in_b=ib, prec="f32")
    assert (st == onp.ST_SKIPPED_SMALL_DT).all() and np.array_equal(g32[1], g32[0]) and np.array_equal(h32[1], h32[0])
