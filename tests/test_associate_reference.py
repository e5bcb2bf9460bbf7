"""tests/associate_reference.py, the float64 statement of the sensor-frame association, pinned without a GPU: K = 1 is
sensor_meas_reference.update_sensor array for array; one hypothesis does not depend on the order of its candidates; the
constructed maps the GPU tests decide on are separated (the conditions are asserted HERE, on the inputs, so that a decision on
the device cannot hinge on rounding); ties go to the lower index; n_gated is a brute-force count; the status rules."""
import numpy as np
import pytest

import associate_reference as ar
import feature_scaled_parity as fsp
import sensor_meas_reference as sr
from engine_support import man_of, same
from oracle import ukf_numpy as on

N = 48
ST_NONFINITE, ST_CHOLESKY, ST_NOCONV, ST_UNINIT, ST_INACTIVE, ST_REJECTED = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8, 1 << 9
FLOATS = ("z_pred", "S", "innov", "maha", "loglik")


def inputs(spe, model, n=N, seed=5):
    """the batch of tests/test_gpu_associate.py on the oracle's cycled state: tests/sensor_meas_cases.make_inputs, and
    OrientationState's nav-frame vectors of length 1 ... 3 (acase of that file)"""
    mu, cov = fsp.cycled_state(spe, model, n)
    rng = np.random.default_rng(seed)
    mount = np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)), on.so3_exp(rng.uniform(-1.0, 1.0, (n, 3)))], axis=1)
    d = rng.standard_normal((n, 3))
    away = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(15.0, 80.0, (n, 1))
    point = (mu[:, 0:3] + away) if model == "pose" else away / np.linalg.norm(away, axis=1, keepdims=True) * rng.uniform(1.0, 3.0, (n, 1))
    gyro = 0.1 * rng.standard_normal((n, 3))
    z = {}
    for mid in sr.ids_of(man_of(model)):
        zz = np.zeros((n, 3))
        zz[:, :sr.meas_dim(mid)] = sr.h(mid, mu, mount, point, gyro) + 0.05 * rng.standard_normal((n, sr.meas_dim(mid)))
        z[mid] = zz
    Q = np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)).copy()
    return mu, cov, mount, point, gyro, z, Q


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_one_candidate_is_update_sensor(spe, model):
    man = man_of(model)
    mu, cov, mount, point, gyro, z, Q = inputs(spe, model)
    ids = np.array(list(sr.ids_of(man)) + [-1], dtype=np.int64)[np.arange(N) % (len(sr.ids_of(man)) + 1)]
    zz = np.zeros((N, 3))
    for mid in sr.ids_of(man):
        zz[ids == mid] = z[mid][ids == mid]
    zz[4, 0] = np.nan                       # an absent only candidate
    cov = cov.copy()
    cov[6] = -np.eye(man.D)                 # a covariance that does not factorise
    init = np.ones(N, bool)
    init[8] = False
    free = sr.update_sensor(man, mu, cov, ids, zz, Q, mount, point, gyro, initialised=init)
    for gate in (-1.0, float(np.nanmedian(free["maha"]))):
        ref = sr.update_sensor(man, mu, cov, ids, zz, Q, mount, point, gyro, gate_chi2=gate, initialised=init)
        for hyp in (False, True):
            got = ar.associate_sensor(man, mu, cov, ids, zz[None], Q, mount, point[None] if hyp else point, gyro, point_per_candidate=hyp,
                                      gate_chi2=gate, initialised=init)
            assert same({k: got[k][0] for k in FLOATS}, ref, FLOATS), (gate, hyp)
            assert same(got, ref, ("mu", "cov", "status")), (gate, hyp)
            good = (ref["status"] & ~np.uint32(ST_NOCONV)) == 0
            assert np.array_equal(got["best"], np.where(good, 0, -1)) and np.array_equal(got["n_gated"], good.astype(np.int32))
        assert ref["status"][4] == ST_NONFINITE and ref["status"][6] == ST_CHOLESKY and ref["status"][8] == ST_UNINIT
    assert (ref["status"] == ST_REJECTED).sum() > N // 4 and (ref["status"][ids < 0] == ST_INACTIVE).all()
    dry = ar.associate_sensor(man, mu, cov, ids, zz[None], Q, mount, point, gyro, initialised=init, commit=False)
    assert np.array_equal(dry["mu"], mu) and np.array_equal(dry["cov"], cov) and same(dry, ar.associate_sensor(
        man, mu, cov, ids, zz[None], Q, mount, point, gyro, initialised=init), FLOATS + ("best", "n_gated", "status"))


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_shared_hypothesis_does_not_depend_on_the_candidate_order(spe, model):
    man = man_of(model)
    mu, cov, mount, point, gyro, z, Q = inputs(spe, model)
    rng = np.random.default_rng(3)
    for mid in sr.ids_of(man):
        zs, _, truth = ar.constructed_candidates(man, mu, cov, mid, z[mid], Q, mount, point, gyro, 5, False)
        zs[1, 9, 0] = np.nan               # a ragged list: an absent candidate, here the filter's first scored one moves
        perm = rng.permutation(5)
        a = ar.associate_sensor(man, mu, cov, mid, zs, Q, mount, point, gyro)
        b = ar.associate_sensor(man, mu, cov, mid, zs[perm], Q, mount, point, gyro)
        assert same(a, b, ("z_pred", "S", "mu", "cov", "n_gated", "status")) and a["z_pred"].shape == (1, N, 3)
        assert same({k: a[k][perm] for k in ("innov", "maha", "loglik")}, b, ("innov", "maha", "loglik"))
        assert np.array_equal(perm[b["best"]], a["best"]) and np.isnan(a["maha"][1, 9]) and a["status"][9] == 0
        expect = truth.copy()
        assert np.array_equal(np.delete(a["best"], 9), np.delete(expect, 9))


@pytest.mark.parametrize("hyp", [False, True])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_constructed_maps_are_separated(spe, model, hyp):
    """three landmarks (or three detections), the true one at index 0, 1 or 2: the reference picks it for every filter, the
    clutter is at least 6 sigma away by the reference's own d^2, and the two smallest d^2 differ by far more than 10 %.  K = 4
    (the GPU parity test's) and the storage types of both engines are held to the same conditions."""
    man = man_of(model)
    mu, cov, mount, point, gyro, z, Q = inputs(spe, model)
    for K, dtype in ((3, np.float64), (4, np.float64), (4, np.float32)):
        for mid in sr.ids_of(man):
            zs, pts, truth = ar.constructed_candidates(man, mu, cov, mid, z[mid], Q, mount, point, gyro, K, hyp, dtype)
            assert set(truth) == set(range(K))
            ref = ar.associate_sensor(man, mu, cov, mid, zs, Q, mount, pts, gyro, point_per_candidate=hyp)
            assert (ref["status"] == 0).all() and np.array_equal(ref["best"], truth), mid
            d2 = np.sort(ref["maha"], axis=0)
            clutter = np.where(np.arange(K)[:, None] == truth[None, :], np.inf, ref["maha"])
            assert clutter.min() >= 36.0, (mid, clutter.min())
            assert (d2[1] > 1.1 * d2[0]).all() and np.array_equal(d2[0], ref["maha"][truth, np.arange(N)])
            assert (ref["n_gated"] == K).all()
            # a gate between the true candidate and the clutter, 10 % clear of both: one candidate inside
            lo, hi = float(d2[0].max()), float(d2[1].min())
            assert 1.1 * lo < hi / 1.1
            gate = float(np.sqrt(lo * hi))
            g = ar.associate_sensor(man, mu, cov, mid, zs, Q, mount, pts, gyro, point_per_candidate=hyp, gate_chi2=gate)
            assert np.array_equal(g["best"], truth) and (g["n_gated"] == 1).all() and same(g, ref, ("mu", "cov", "maha"))
            # a gate below every d^2: REJECTED_GATE, the scores stay, the state too
            g = ar.associate_sensor(man, mu, cov, mid, zs, Q, mount, pts, gyro, point_per_candidate=hyp, gate_chi2=0.5 * float(d2[0].min()))
            assert (g["status"] == ST_REJECTED).all() and (g["best"] == -1).all() and (g["n_gated"] == 0).all()
            assert same(g, ref, FLOATS) and np.array_equal(g["mu"], mu) and np.array_equal(g["cov"], cov)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_ties_go_to_the_lower_index_and_n_gated_counts(spe, model):
    man = man_of(model)
    mu, cov, mount, point, gyro, z, Q = inputs(spe, model)
    mid = sr.ids_of(man)[-2]   # POSE_VELOCITY / ORIENT_NAV_VECTOR
    K = 32
    rng = np.random.default_rng(17)
    zs = z[mid][None] + 0.08 * rng.standard_normal((K, N, 3))
    zs[20] = zs[4]             # duplicated candidates
    zs[9] = zs[30]
    zs[2, ::3] = np.nan        # and a ragged list
    free = ar.associate_sensor(man, mu, cov, mid, zs, Q, mount, point, gyro)
    assert np.array_equal(free["maha"][20], free["maha"][4]) and np.array_equal(free["maha"][9], free["maha"][30])
    assert not np.isin(free["best"], (20, 30)).any()
    for forced, low in ((20, 4), (30, 9)):   # make the duplicated pair the nearest: the true sample itself
        zz = zs.copy()
        zz[forced] = zz[low] = sr_mean(man, mu, cov, mid, Q, mount, point, gyro)
        r = ar.associate_sensor(man, mu, cov, mid, zz, Q, mount, point, gyro)
        assert (r["best"] == low).all() and (r["maha"][low] < 1e-20).all()
    gate = float(np.nanmedian(free["maha"]))
    r = ar.associate_sensor(man, mu, cov, mid, zs, Q, mount, point, gyro, gate_chi2=gate)
    brute = np.array([sum(1 for k in range(K) if np.isfinite(r["maha"][k, i]) and r["maha"][k, i] <= gate) for i in range(N)])
    assert np.array_equal(r["n_gated"], brute) and brute.min() >= 1 and brute.max() < K - 1 and len(set(brute)) > 3
    assert np.array_equal(free["n_gated"], np.isfinite(free["maha"]).sum(axis=0)) and set(free["n_gated"]) == {K - 1, K}
    for i in range(N):
        inside = [k for k in range(K) if np.isfinite(r["maha"][k, i]) and r["maha"][k, i] <= gate]
        assert r["best"][i] == min(inside, key=lambda k: (r["maha"][k, i], k))


def sr_mean(man, mu, cov, mid, Q, mount, point, gyro):
    """z-bar of every filter: a sample with innovation zero"""
    return sr.update_sensor(man, mu, cov, mid, np.zeros((mu.shape[0], 3)), Q, mount, point, gyro)["z_pred"]


def test_status_rules(spe):
    man = on.POSE
    mu, cov, mount, point, gyro, z, Q = inputs(spe, "pose")
    mid, K = sr.POSE_POINT, 3
    zs, pts, truth = ar.constructed_candidates(man, mu, cov, mid, z[mid], Q, mount, point, gyro, K, True)
    zs, pts, Qb, mb = zs.copy(), pts.copy(), Q.copy(), mount.copy()
    zs[:, 1] = np.nan                       # every candidate absent
    zs[truth[2], 2, 1] = np.nan             # the true candidate absent: the nearest clutter is taken
    pts[truth[4], 4, 2] = np.inf            # per hypothesis: a non-finite point makes its candidate absent
    pts[:, 6, 0] = np.nan
    Qb[8, 1, 0] = np.nan
    mb[10, 5] = np.nan
    r = ar.associate_sensor(man, mu, cov, mid, zs, Qb, mb, pts, gyro, point_per_candidate=True)
    expect = np.zeros(N, dtype=np.uint32)
    expect[[1, 6, 8, 10]] = ST_NONFINITE
    assert np.array_equal(r["status"], expect)
    bad = expect != 0
    assert all(np.isnan(r[k][:, bad]).all() for k in FLOATS) and (r["best"][bad] == -1).all() and (r["n_gated"][bad] == 0).all()
    assert np.array_equal(r["mu"][bad], mu[bad]) and not np.array_equal(r["mu"][0], mu[0])
    for i in (2, 4):
        assert r["best"][i] != truth[i] and r["best"][i] >= 0 and r["n_gated"][i] == K - 1
        assert np.isnan(r["maha"][truth[i], i]) and np.isnan(r["z_pred"][truth[i], i]).all() and np.isnan(r["S"][truth[i], i]).all()
    ok = ~bad & ~np.isin(np.arange(N), (2, 4))
    assert np.array_equal(r["best"][ok], truth[ok])
    # the same points handed to a model that does not read them: the flag has no effect
    a = ar.associate_sensor(man, mu[ok], cov[ok], sr.POSE_VELOCITY, zs[:, ok], Q[ok], mount[ok], pts[:, ok] * np.nan, gyro[ok], point_per_candidate=True)
    b = ar.associate_sensor(man, mu[ok], cov[ok], sr.POSE_VELOCITY, zs[:, ok], Q[ok], mount[ok], np.zeros(3), gyro[ok])
    assert same(a, b, ("innov", "maha", "loglik", "best", "n_gated", "status", "mu", "cov")) and (a["status"] == 0).all()
    assert all(same({k: a[k][j] for k in ("z_pred", "S")}, {k: b[k][0] for k in ("z_pred", "S")}, ("z_pred", "S")) for j in range(K))
