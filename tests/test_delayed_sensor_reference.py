"""Pins tests/delayed_sensor_reference.py, the NumPy statement of the late sensor-frame samples
(include/ukf_batch_delayed_sensor.h), on the CPU: the yardstick of tests/test_gpu_delayed_sensor.py must itself be right.  The
figures the tests print are kept in profiles/delayed_sensor_parity.txt and DESIGN.md 4.29."""
import numpy as np
import pytest

import delayed_reference as dr
import delayed_sensor_cases as dc
import delayed_sensor_reference as dsr
import scaled_parity as sp
import sensor_meas_cases as smc
import sensor_meas_reference as smr
import smoother_reference as sr
from engine_support import man_of, scaled, scaled_ignoring_nan
from oracle import ukf_numpy as on

STEPS = dc.STEPS
KEYS = ("mu", "cov", "z_pred", "S", "innov", "maha", "loglik")

_HIST = {}


def hist(spe, model, n=64):
    if (model, n) not in _HIST:
        _HIST[(model, n)] = dc.cpu_history(spe, model, n, STEPS)
    return _HIST[(model, n)]


def call_at(spe, model, n, lag, ids=None, identity=False):
    """a late sample of every filter at lag `lag` on the hot CPU history -> (reference result, arguments)"""
    p, mu, cov, dt, ia, ib, _ = hist(spe, model, n)
    ids = dc.cycling_ids(model, n) if ids is None else ids
    mu_s = dc.state_at_lag(mu, mu[-1], lag)
    mount = np.broadcast_to(smr.IDENTITY_MOUNT, (n, 7)).copy() if identity else dc.mounts(n)
    point = np.zeros((n, 3)) if identity else dc.points(model, n, mu_s)
    w = dc.rates(n)
    z = dc.samples(spe, model, ids, mu_s, mount, point, w)
    args = dict(p=p, mu=mu, cov=cov, dt=dt, lag=lag, ids=ids, z=z, mount=mount, point=point, w=w, ia=ia, ib=ib)
    r = dsr.update_delayed_sensor(p, mu, cov, mu[-1], cov[-1], dt, lag, ids, z, dc.Q_SAMPLE, mount, point, rate=w, in_a=ia,
                                  in_b=ib if model == "orient" else None)
    return r, args


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_lag_zero_is_the_sensor_frame_update(model):
    """all eight models: with lag 0 the chain is empty, M = I, and the call is sensor_meas_reference.update_sensor on the
    present state"""
    n = 64
    mu, cov, gyro = smc.states(model)
    mu, cov = mu[:n], cov[:n]
    gyro = np.zeros((n, 3)) if gyro is None else gyro[:n]
    mount = dc.mounts(n)
    point = dc.points(model, n, mu)
    p = sr.Params("pose", np.eye(12)) if model == "pose" else sr.Params("orient", np.eye(13))
    worst = 0.0
    for mid in smr.ids_of(man_of(model)):
        z = np.zeros((n, 3))
        z[:, :smr.meas_dim(mid)] = smr.h(mid, mu, mount, point, gyro) + 0.03
        a = dsr.update_delayed_sensor(p, mu[None], cov[None], mu, cov, [], 0, mid, z, dc.Q_SAMPLE, mount, point, rate=gyro)
        b = smr.update_sensor(man_of(model), mu, cov, mid, z, dc.Q_SAMPLE, mount, point, gyro)
        assert (a["status"] == 0).all() and (b["status"] == 0).all() and a["committed"].all()
        m = smr.meas_dim(mid)
        assert (a["z_pred"][:, m:] == 0).all() and a["z_pred"].shape == (n, 4)
        figs = {k: scaled(a[k][:, :3] if k == "z_pred" else a[k], b[k]) for k in KEYS}
        print(f"DELAYED-SENSOR lag 0 against update_sensor, {smr.NAMES[mid]}: " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
        worst = max(worst, max(figs.values()))
    assert worst <= 1e-12


@pytest.mark.parametrize("lag", [1, 2, 5])
def test_identity_mount_is_the_delayed_update_with_model_0(spe, lag):
    """POSE_POSITION with r = 0 (and b = 0): h(X) = p + R(q) 0 = p, the delayed update's model 0 on the same chain"""
    n = 64
    a, g = call_at(spe, "pose", n, lag, ids=np.full(n, smr.POSE_POSITION, np.int32), identity=True)
    b = dr.update_delayed(g["p"], g["mu"], g["cov"], g["mu"][-1], g["cov"][-1], g["dt"], lag, on.MEAS_POS3, g["z"], dc.Q_SAMPLE, in_a=g["ia"])
    assert (a["status"] == 0).all() and (b["status"] == 0).all() and a["committed"].all() and b["committed"].all()
    figs = {k: scaled(a[k], b[k]) for k in KEYS + ("mu_out", "cov_out")}
    print(f"DELAYED-SENSOR identity mount against delayed model 0, lag {lag}: " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    assert max(figs.values()) <= 1e-12


def in_order(spe, model, n, s, mid, z, mount, point, w):
    """the sample processed at its own step s by the sensor-frame update, then the recorded cycles up to the present"""
    p, mu, cov, dt, _, _, inputs = hist(spe, model, n)
    r = smr.update_sensor(man_of(model), mu[s], cov[s], mid, z, dc.Q_SAMPLE, mount, point, w)
    assert (r["status"] == 0).all()
    m, C = r["mu"], r["cov"]
    for c in range(s + 1, STEPS):
        _, _, cm, cz, cQ = inputs[c]
        m, C = dc.cpu_cycle(p, m, C, inputs[c - 1][0], inputs[c - 1][1], dt[c - 1], cm, cz, cQ)
    return m, C


def state_distance(model, mu, mu_ref, cov_ref):
    """[n]: |mu (-) mu_ref| in units of the reference's own sigmas, the largest component of every filter"""
    d = man_of(model).boxminus(mu, mu_ref)
    return np.max(np.abs(d) / np.sqrt(np.einsum("nii->ni", cov_ref)), axis=1)


@pytest.mark.parametrize("mid", [smr.POSE_POSITION, smr.POSE_POINT], ids=["POSE_POSITION", "POSE_POINT"])
def test_the_call_beats_what_a_caller_could_do_before(spe, mid):
    """254 filters of the hot history, a sample taken 3 steps ago: the distance to the in-order result of (a) this call, (b)
    the body-origin workaround z - R(q_n) r into the delayed update's model 0 (POSE_POSITION only) and (c) dropping the sample.
    Asserted: the median of (a) is below that of (b) and of (c), and nothing more.  Measured, medians / worst
    filter in sigmas of the in-order state: POSE_POSITION (a) 1.17e-02 / 5.43e-02, (b) 3.85e-01 / 1.41e+00, (c) 3.85e-01 /
    1.40e+00 -- the workaround is no better than dropping the fix; POSE_POINT (a) 6.71e-03 / 1.17e-01, (c) 5.20e-01 / 3.68e+00."""
    n, lag = 254, 3
    s = STEPS - 1 - lag
    p, mu, cov, dt, ia, _, _ = hist(spe, "pose", n)
    mount = dc.mounts(n, lever=1.0)
    point = dc.points("pose", n, mu[s])
    ids = np.full(n, mid, np.int32)
    z = dc.samples(spe, "pose", ids, mu[s], mount, point)
    mu_io, cov_io = in_order(spe, "pose", n, s, mid, z, mount, point, np.zeros((n, 3)))
    a = dsr.update_delayed_sensor(p, mu, cov, mu[-1], cov[-1], dt, lag, ids, z, dc.Q_SAMPLE, mount, point, in_a=ia)
    assert (a["status"] == 0).all() and a["committed"].all()
    cand = {"a: this call": a["mu"], "c: sample dropped": mu[-1]}
    if mid == smr.POSE_POSITION:
        zb = z - on.quat_rotate(mu[-1][:, 3:7], mount[:, 0:3])   # the fix moved to the body origin with the PRESENT orientation
        b = dr.update_delayed(p, mu, cov, mu[-1], cov[-1], dt, lag, on.MEAS_POS3, zb, dc.Q_SAMPLE, in_a=ia)
        assert (b["status"] == 0).all()
        cand["b: body-origin workaround"] = b["mu"]
    med = {}
    for k, m in cand.items():
        d = state_distance("pose", m, mu_io, cov_io)
        med[k[0]] = np.median(d)
        print(f"DELAYED-SENSOR claim {smr.NAMES[mid]} lag {lag}, distance to in-order in its sigmas, {k}: median {np.median(d):.3e} "
              f"worst {d.max():.3e} (filter {int(d.argmax())})")
    assert med["a"] < med["c"]
    if "b" in med:
        assert med["a"] < med["b"]


def test_status_rules(spe):
    n = 32
    lag = np.arange(n) % STEPS
    for model in ("pose", "orient"):
        clean, g = call_at(spe, model, n, lag)
        assert (clean["status"] == 0).all() and clean["committed"].all()
        own = smr.ids_of(man_of(model))
        other = smr.ORIENT_VELOCITY if model == "pose" else smr.POSE_POSITION
        lag2, ids2, z2 = lag.copy(), g["ids"].copy(), g["z"].copy()
        mount2, point2, w2 = g["mount"].copy(), g["point"].copy(), g["w"].copy()
        live = np.ones(n, bool)
        live[0] = False
        lag2[1], lag2[2] = -1, STEPS
        ids2[3], ids2[4], ids2[5] = other, -1, 8
        # NaN in an entry the model reads (z[0], the lever arm of a model that has one) and in entries it does not
        z2[6, 0] = np.nan
        lever = smr.POSE_POSITION if model == "pose" else smr.ORIENT_VELOCITY
        ids2[7] = lever
        z2[7] = dc.samples(spe, model, ids2, dc.state_at_lag(g["mu"], g["mu"][-1], lag2), mount2, point2, w2)[7]
        mount2[7, 1] = np.inf
        nolever = smr.POSE_NAV_VELOCITY if model == "pose" else smr.ORIENT_SPECIFIC_FORCE
        ids2[8] = nolever
        z2[8] = dc.samples(spe, model, ids2, dc.state_at_lag(g["mu"], g["mu"][-1], lag2), mount2, point2, w2)[8]
        mount2[8], point2[8], w2[8] = np.nan, np.nan, np.nan
        if model == "orient":
            ids2[9] = smr.ORIENT_VELOCITY
            w2[9, 2] = np.nan
        z2[10] += 40.0   # gated
        # a poisoned record inside the chain of filter 11 (lag 3: steps 4, 3, 2) and the same poison below the chain of filter 12
        mu2, cov2 = g["mu"].copy(), g["cov"].copy()
        lag2[11], lag2[12] = 3, 1
        for i in (11, 12):
            ids2[i] = own[0]
        z2[[11, 12]] = dc.samples(spe, model, ids2, dc.state_at_lag(mu2, mu2[-1], lag2), mount2, point2, w2)[[11, 12]]
        cov2[3, 11] = -np.eye(cov2.shape[-1])
        cov2[3, 12] = -np.eye(cov2.shape[-1])
        r = dsr.update_delayed_sensor(g["p"], mu2, cov2, mu2[-1], cov2[-1], g["dt"], lag2, ids2, z2, dc.Q_SAMPLE, mount2, point2, rate=w2,
                                      in_a=g["ia"], in_b=g["ib"] if model == "orient" else None, initialised=live, gate_chi2=9.0)
        st = r["status"]
        want = {0: on.ST_UNINITIALISED, 1: on.ST_INACTIVE, 2: on.ST_ERR_NEG_DT, 3: on.ST_INACTIVE, 4: on.ST_INACTIVE, 5: on.ST_INACTIVE,
                6: on.ST_ERR_NONFINITE_MEAS, 7: on.ST_ERR_NONFINITE_MEAS, 8: 0, 10: on.ST_REJECTED_GATE, 11: on.ST_ERR_CHOLESKY, 12: 0}
        if model == "orient":
            want[9] = on.ST_ERR_NONFINITE_MEAS
        for i, s in want.items():
            assert st[i] == s, (model, i, st[i], s)
        quiet = [i for i, s in want.items() if s != 0]
        assert not r["committed"][quiet].any() and np.isnan(r["mu_out"][quiet]).all()
        assert np.array_equal(r["mu"][quiet], mu2[-1][quiet]) and np.array_equal(r["cov"][quiet], cov2[-1][quiet])
        assert np.isfinite(r["maha"][10]) and np.isfinite(r["S"][10]).all() and np.isnan(r["maha"][[0, 1, 2, 6, 11]]).all()
        assert r["committed"][[8, 12]].all() and np.isfinite(r["mu_out"][[8, 12]]).all()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_fp32_study(spe, model):
    """delayed_sensor_f32 with every stage float64 is the reference; with every stage float32 its distance, block by block, is
    the d_32 that feeds feature_scaled_parity.judge_state"""
    n = 64
    lag = np.arange(n) % STEPS
    r, g = call_at(spe, model, n, lag)
    ib = g["ib"] if model == "orient" else None
    args = (g["p"], g["mu"], g["cov"], g["mu"][-1], g["cov"][-1], g["dt"], lag, g["ids"], g["z"], dc.Q_SAMPLE, g["mount"], g["point"], g["w"],
            g["ia"], ib)
    m64, C64 = dsr.delayed_sensor_f32(*args, prec="f64")
    e64 = max(scaled(m64, r["mu"]), scaled(C64, r["cov"]))
    m32, C32 = dsr.delayed_sensor_f32(*args, prec="f32")
    em, ec = scaled_ignoring_nan(m32, m64), scaled_ignoring_nan(C32, C64)
    print(f"DELAYED-SENSOR {model} float64 stages against the reference {e64:.3e}; float32 evaluation: mean {em:.3e} cov {ec:.3e}")
    print(sp.table(sp.distances(model, m32, C32, m64, C64)))
    assert e64 <= 1e-12
    assert em <= 1e-4 / 7.0 and ec <= 1e-4 / 7.0   # the gate with feature_scaled_parity's margin M_FEAT to spare
