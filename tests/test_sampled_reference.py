"""Pins for tests/sampled_reference.py, the NumPy statement of the user-defined measurement models (include/ukf_batch.h) the GPU
tests compare with: fed the samples of a built-in sensor model it returns what tests/sensor_meas_reference.py returns, a
translation of z and Z moves z-bar and nothing else, the status rules hold one by one, and the GPU file's input family gives
status 0 for every filter not deliberately broken.  (That a linear h gives the closed-form Kalman update is pinned where the
arithmetic lives, in tests/test_update_reference.py.)"""
import numpy as np
import pytest

import sampled_reference as sm
import sensor_meas_reference as sr
from engine_support import man_of
from oracle import ukf_numpy as on
from sensor_meas_cases import mounts, states

N = 1022


# ------------------------------------------------------------------------------------------------------------------ export
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_export_layout(model):
    man = man_of(model)
    mu, cov, _ = states(model)
    mu, cov = mu[:64], cov[:64]
    X, delta, st = sm.sigma_points(man, mu, cov)
    assert X.shape == (64, 2 * man.D + 1, man.S) and delta.shape == (64, 2 * man.D + 1, man.D) and (st == 0).all()
    Xo, ok = on.sigma_points(man, mu, cov)
    assert ok.all() and np.array_equal(X[:, 1:], Xo[:, 1:]) and np.array_equal(X[:, 0], mu)
    L, _ = on.cholesky_lower(cov)
    for j in range(man.D):
        assert np.array_equal(delta[:, 1 + 2 * j], L[:, :, j]) and np.array_equal(delta[:, 2 + 2 * j], -L[:, :, j])
    assert (delta[:, 0] == 0).all()
    assert np.array_equal(man.boxplus(mu[:, None, :], delta)[:, 1:], X[:, 1:])   # X = mu (+) delta
    # a filter without points
    init = np.ones(64, bool)
    init[5] = False
    bad = cov.copy()
    bad[9] = -np.eye(man.D)
    X2, d2, st2 = sm.sigma_points(man, mu, bad, initialised=init)
    assert st2[5] == on.ST_UNINITIALISED and st2[9] == on.ST_ERR_CHOLESKY and (np.delete(st2, [5, 9]) == 0).all()
    assert np.isnan(X2[[5, 9]]).all() and np.isnan(d2[[5, 9]]).all()
    keep = np.delete(np.arange(64), [5, 9])
    assert np.array_equal(X2[keep], X[keep]) and np.array_equal(d2[keep], delta[keep])


# --------------------------------------------------------------------------------------------- the built-in sensor models
@pytest.mark.parametrize("mid", [0, 1, 2, 6])
def test_samples_of_a_sensor_model_give_the_sensor_reference(mid):
    model = "pose" if mid <= 4 else "orient"
    man = man_of(model)
    mu, cov, gyro = states(model)
    mount, rng = mounts(N)
    d = rng.standard_normal((N, 3))
    away = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(15.0, 80.0, (N, 1))
    point = mu[:, 0:3] + away if model == "pose" else away
    gyro = np.zeros((N, 3)) if gyro is None else gyro
    m = sr.meas_dim(mid)
    z = np.zeros((N, 3))
    z[:, :m] = sr.h(mid, mu, mount, point, gyro) + 0.05 * rng.standard_normal((N, m))
    Q = np.broadcast_to(0.05 ** 2 * np.eye(3), (N, 3, 3))
    gate = -1.0   # POSE_POINT: with a gate at the median of the ungated d^2
    if mid == 2:
        gate = float(np.median(sr.update_sensor(man, mu, cov, mid, z, Q, mount, point, gyro)["maha"]))
    ref = sr.update_sensor(man, mu, cov, mid, z, Q, mount, point, gyro, gate_chi2=gate)
    _, uq, um, up = sr.used_inputs(mid)
    mt = np.where(um, mount, sr.IDENTITY_MOUNT)[:, None, :]
    pt = np.where(up, point, 0.0)[:, None, :]
    Z = sr.h(mid, on.sigma_points(man, mu, cov)[0], mt, pt, gyro[:, None, :])
    got = sm.update_sampled(man, mu, cov, Z, z[:, :m], Q[:, :m, :m], gate_chi2=gate)
    assert np.array_equal(got["status"], ref["status"])
    if mid == 2:
        assert (ref["status"] == on.ST_REJECTED_GATE).any() and (ref["status"] == 0).any()
    else:
        assert (ref["status"] == 0).all()
    for k in ("mu", "cov", "maha", "loglik"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["z_pred"], ref["z_pred"][:, :m]) and np.array_equal(got["innov"], ref["innov"][:, :m])
    assert np.array_equal(got["S"], ref["S"][:, :m, :m])


# ------------------------------------------------------------------------------------------------------- the user family
_FAMILY = {}


def family(model, m):
    if (model, m) not in _FAMILY:
        man = man_of(model)
        mu, cov, _ = states(model)
        b, r, noise, Q = sm.make_inputs(model, mu, np.float64)
        X, _, st = sm.sigma_points(man, mu, cov)
        assert (st == 0).all()
        Z = sm.user_h(model, m, X, b[:, None, :], r[:, None, :])
        z = sm.user_h(model, m, mu, b, r) + noise[m]
        _FAMILY[(model, m)] = (mu, cov, Z, z, Q[m])
    return _FAMILY[(model, m)]


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_gpu_input_family_gives_status_zero(model):
    """every m of the GPU file's family, float64 and float32 storage of the inputs: status 0 for every filter and a real update"""
    man = man_of(model)
    for m in sm.USER_DIMS:
        mu, cov, Z, z, Q = family(model, m)
        assert Z.shape == (N, 2 * man.D + 1, m) and np.array_equal(Q, np.swapaxes(Q, 1, 2))
        for dt in (np.float64, np.float32):
            st = lambda x: x.astype(dt).astype(np.float64)   # noqa: E731
            o = sm.update_sampled(man, mu, cov, st(Z), st(z), st(Q))
            assert (o["status"] == 0).all(), (m, dt, np.unique(o["status"]))
            assert not np.array_equal(o["mu"], mu) and np.isfinite(o["loglik"]).all()
        print(f"{model} m={m}: mean d^2 = {o['maha'].mean():.3f}, max = {o['maha'].max():.3f}")
        assert (o["maha"] > 0).all() and np.isfinite(o["maha"]).all()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_translation_moves_only_z_pred(model):
    """z and all Z_i translated by a per-filter constant t (|t| <= 1000): z-bar moves by t; everything else is a function of the
    differences Z_i - Z_0 and z - Z_0 alone.  In float64 absolute coordinates (the oracle's) those differences carry the rounding
    of |t| eps ~ 2e-13 against deltas of centimetres and more, amplified by the condition of S (up to ~ 1e4 in this family):
    1e-8 on the scaled outputs"""
    man = man_of(model)
    m = 4
    mu, cov, Z, z, Q = family(model, m)
    t = np.random.default_rng(3).uniform(-1000.0, 1000.0, (N, m))
    a = sm.update_sampled(man, mu, cov, Z, z, Q)
    b = sm.update_sampled(man, mu, cov, Z + t[:, None, :], z + t, Q)
    assert np.array_equal(a["status"], b["status"]) and (a["status"] == 0).all()
    worst = max(float(np.max(np.abs(a[k] - b[k]) / (1.0 + np.abs(a[k])))) for k in ("mu", "cov", "S", "innov", "maha", "loglik"))
    dz = np.abs(b["z_pred"] - (a["z_pred"] + t)).max()
    print(f"{model}: translation by up to 1000: max scaled change {worst:.3e}, z_pred - (z_pred + t) {dz:.3e}")
    assert worst <= 1e-8 and dz <= 1e-9
    assert np.abs(b["z_pred"] - a["z_pred"]).max() > 100.0


def test_status_rules_one_by_one():
    man, m = on.POSE, 3
    mu, cov, Z, z, Q = (x[:16].copy() for x in family("pose", m))
    clean = sm.update_sampled(man, mu, cov, Z, z, Q)
    assert (clean["status"] == 0).all()

    def only(i, st, **kw):
        o = sm.update_sampled(man, kw.pop("mu", mu), kw.pop("cov", cov), kw.pop("Z", Z), kw.pop("z", z), kw.pop("Q", Q), **kw)
        want = np.zeros(16, dtype=np.uint32)
        want[i] = st
        assert np.array_equal(o["status"], want), (o["status"], want)
        rest = np.arange(16) != i
        for k in clean:
            assert np.array_equal(o[k][rest], clean[k][rest]), k
        return o
    init = np.ones(16, bool)
    init[3] = False
    o = only(3, on.ST_UNINITIALISED, initialised=init)
    assert np.array_equal(o["mu"][3], mu[3]) and np.isnan(o["maha"][3]) and np.isnan(o["z_pred"][3]).all()
    act = np.ones(16, np.uint8)
    act[4] = 0
    o = only(4, on.ST_INACTIVE, active=act)
    assert np.array_equal(o["cov"][4], cov[4]) and np.isnan(o["S"][4]).all()
    act[3] = 0
    assert sm.update_sampled(man, mu, cov, Z, z, Q, active=act, initialised=init)["status"][3] == on.ST_UNINITIALISED
    for what in ("Z", "z", "Q"):
        x = {"Z": Z, "z": z, "Q": Q}[what].copy()
        x[5].flat[-1 if what != "Q" else 3] = np.nan   # Q: entry (1, 0), in the lower triangle
        o = only(5, on.ST_ERR_NONFINITE_MEAS, **{what: x})
        assert np.array_equal(o["mu"][5], mu[5]) and np.isnan(o["loglik"][5])
    Qu = Q.copy()
    Qu[5, 0, 2] = np.nan   # the upper triangle is not read
    o = sm.update_sampled(man, mu, cov, Z, z, Qu)
    for k in clean:
        assert np.array_equal(o[k], clean[k]), k
    bad = cov.copy()
    bad[6] = -np.eye(12)
    only(6, on.ST_ERR_CHOLESKY, cov=bad)
    Qn = Q.copy()
    Qn[7] = -1e6 * np.eye(m)
    o = only(7, on.ST_ERR_CHOLESKY, Q=Qn)
    assert np.array_equal(o["mu"][7], mu[7]) and np.isnan(o["maha"][7])
    gate = float(np.median(clean["maha"]))
    o = sm.update_sampled(man, mu, cov, Z, z, Q, gate_chi2=gate)
    rej = clean["maha"] > gate
    assert rej.any() and (~rej).any() and np.array_equal(o["status"], np.where(rej, on.ST_REJECTED_GATE, 0))
    assert np.array_equal(o["mu"][rej], mu[rej]) and np.array_equal(o["maha"], clean["maha"]) and np.array_equal(o["mu"][~rej], clean["mu"][~rej])
    o = sm.update_sampled(man, mu, cov, Z, z, Q, max_it=1)
    assert (o["status"] == on.ST_WARN_MEAN_NOCONV).all()
