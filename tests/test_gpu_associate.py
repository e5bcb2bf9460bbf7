"""Sensor-frame association on the device (ukfb_associate_sensor_dev / ukfb_associate_sensor, include/ukf_batch.h).

States, inputs, engines, the three precision modes and their tolerances are those of tests/test_gpu_sensor_meas.py (tests/sensor_meas_cases.py:
PRECS, case, engine_of, make_inputs), but for the length of OrientationState's nav-frame vectors (acase below).  Candidates are the constructed maps of
tests/associate_reference.constructed_candidates -- the true candidate of filter i at index i % K, clutter at least 6 sigma
away -- whose separation tests/test_associate_reference.py asserts on the inputs, so that no decision here hinges on rounding.
The reference is tests/associate_reference.py on the state AS DOWNLOADED and the inputs AS STORED.  Parity bound:
|x - ref| <= tol (1 + |ref|) on mean, covariance, z-bar, S, nu, d^2 and log-likelihood; best, n_gated and status are equal.
Every comparison prints a PARITY line before it asserts, and makes the scaled checks of tests/feature_scaled_parity.py
(judge_state on the committed state, judge_meas on z-bar, S and nu of every hypothesis); a plain fp32 engine's bound comes from
the all-float32 evaluation of the same calls (tests/feature_f32.sensor_meas, once per candidate)."""
import numpy as np
import pytest
import torch

import associate_reference as ar
import feature_f32 as ff
import feature_scaled_parity as fsp
import sensor_meas_cases as smc
import sensor_meas_reference as sr
from engine_support import cycled_engine, man_of, same_snapshot, scaled, snapshot, stored, tdt
from sensor_meas_cases import PRECS, case, cycling_ids, engine_of

pytestmark = pytest.mark.gpu

K4 = 4
ST_NONFINITE, ST_CHOLESKY, ST_UNINIT, ST_INACTIVE, ST_REJECTED = 1 << 4, 1 << 5, 1 << 7, 1 << 8, 1 << 9
FLOATS = ("z_pred", "S", "innov", "maha", "loglik")
INTS = ("best", "n_gated", "status")
FILL = -7.0


def run(e, ids, z, Q, mount, point, hyp=False, commit=True, q_uniform=False):
    """-> dict(mu, cov, z_pred [H, n, 3], S [H, n, 3, 3], innov [K, n, 3], maha, loglik [K, n], best, n_gated, status [n])
    after associate_sensor_dev; mount [7] / point [3]: uniform; hyp: point is [K, n, 3]"""
    n, dt, K = e.capacity, tdt(e), int(np.shape(z)[0])
    H = K if hyp else 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    zd = dev(z)
    qd = dev(np.asarray(Q).reshape(9) if q_uniform else np.asarray(Q).reshape(n, 9))
    idd = None if np.isscalar(ids) else torch.from_numpy(np.asarray(ids, dtype=np.int32)).to("cuda")
    mount, point = np.asarray(mount), np.asarray(point)
    md = dev(mount) if mount.ndim == 2 else None
    pd = dev(point) if point.ndim >= 2 else None
    full = lambda shape, v=FILL, t=dt: torch.full(shape, v, dtype=t, device="cuda")   # noqa: E731
    o = {"z_pred": full((H, n, 3)), "S": full((H, n, 9)), "innov": full((K, n, 3)), "maha": full((K, n)), "loglik": full((K, n)),
         "best": full((n,), -9, torch.int32), "n_gated": full((n,), -9, torch.int32), "status": full((n,), -1, torch.int32)}
    torch.cuda.synchronize()
    e.associate_sensor_dev(int(ids) if idd is None else 0, K, zd, qd, q_is_uniform=q_uniform, model_dev=idd, mount_dev=md,
                           mount=mount if md is None else smc.spe_identity(), point_dev=pd, point=point if pd is None else (0.0, 0.0, 0.0),
                           point_per_candidate=hyp, commit=commit, **o)
    e.sync()
    torch.cuda.synchronize()
    r = {k: o[k].double().cpu().numpy() for k in FLOATS}
    r["S"] = r["S"].reshape(H, n, 3, 3)
    r["best"], r["n_gated"] = o["best"].cpu().numpy(), o["n_gated"].cpu().numpy()
    r["status"] = o["status"].cpu().numpy().astype(np.uint32)
    r["mu"], r["cov"], _ = e.state()
    return r


_ACASE = {}


def acase(spe, model, pname, n=smc.N):
    """The sensor test's case (state after two cycles as downloaded, inputs as stored).  PoseWithVelocity: as it is, landmarks
    and beacons 15 ... 80 m away.  OrientationState: the nav-frame vectors of ORIENT_NAV_VECTOR get the length of catalogue
    entries, 1 ... 3 (a field vector, a star direction), instead of that file's 15 ... 80.  Why: at 15 ... 80 the S of that
    model has condition 500 ... 1700, and a plain fp32 d^2 carries the relative error of the fp32 S times that condition.  The
    sensor test's d^2 of a few units hides it behind the 1 of tol (1 + |ref|); clutter at d^2 of 10^2 ... 10^5 does not.
    Measured on an MI355X with the long vectors: max |d^2 - ref| / (1 + |ref|) = 1.00e-4 (parity, per hypothesis), 1.04e-4 and
    1.18e-4 (gate, shared and per hypothesis) against the 1e-4 of PRECS, every other figure of those runs and both other modes
    within their bounds -- with the fp32 S of the sensor kernel itself (K = 1 equals ukfb_update_sensor_dev bit for bit in
    z-bar, S, nu and d^2).  The bound stays; the vectors are of the size the model is for."""
    c0 = case(spe, model, pname, n)
    if model == "pose":
        return c0
    key = (pname, n)
    if key not in _ACASE:
        c = smc.Case()
        c.__dict__.update(c0.__dict__)
        rng = np.random.default_rng(29)
        c.point = stored(c0.point / np.linalg.norm(c0.point, axis=1, keepdims=True) * rng.uniform(1.0, 3.0, (n, 1)), c.dtype)
        c.z = dict(c0.z)
        mid = sr.ORIENT_NAV_VECTOR
        c.z[mid] = stored(sr.h(mid, c.mu, c.mount, c.point, c.gyro) + 0.05 * rng.standard_normal((n, 3)), c.dtype)
        c.refs = {}
        _ACASE[key] = c
    return _ACASE[key]


def reference(c, ids, zs, pts, hyp, gate=-1.0, **kw):
    return ar.associate_sensor(man_of(c.model), c.mu, c.cov, ids, zs, c.Q, c.mount, pts, c.gyro, point_per_candidate=hyp, gate_chi2=gate, **kw)


def constructed(c, ids, K, hyp):
    """-> (z [K, n, 3], points, truth) for the case's batch, as the engine stores them"""
    z_true = c.z[int(ids)] if np.isscalar(ids) else smc.mixed_z(c, ids)
    return ar.constructed_candidates(man_of(c.model), c.mu, c.cov, ids, z_true, c.Q, c.mount, c.point, c.gyro, K, hyp, c.dtype)


def same_candidates(a, b, keys=("mu", "cov") + FLOATS + INTS, rows=None):
    """bit equality; rows: a selection of filters (the second axis of the per-candidate and per-hypothesis outputs)"""
    rows = slice(None) if rows is None else rows
    part = lambda o, k: o[k][:, rows] if k in FLOATS else o[k][rows]   # noqa: E731
    return all(np.array_equal(part(a, k), part(b, k), equal_nan=True) for k in keys)


def check_parity(name, c, got, ref, ids, zs, pts, hyp, tol=None, state=True):
    tol = c.tol if tol is None else tol
    r = {k: np.asarray(ref[k], dtype=np.float64) for k in ("mu", "cov") + FLOATS}
    if c.wide:   # the engine stores fp32
        r = {k: v.astype(np.float32).astype(np.float64) for k, v in r.items()}
    for k in INTS:
        assert np.array_equal(got[k], ref[k]), (name, k, np.nonzero(got[k] != ref[k])[0][:8])
    for k in ("z_pred", "S", "maha", "loglik"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(r[k])), (name, k)
    assert np.array_equal(np.isnan(got["innov"][..., 0]), np.isnan(r["innov"][..., 0])), name
    err = {k: scaled(got[k], r[k]) for k in ("mu", "cov")} if state else {}
    err.update({k: scaled(got[k][~np.isnan(r[k])], r[k][~np.isnan(r[k])]) for k in FLOATS})
    print(f"PARITY {name} n={c.n} K={zs.shape[0]} " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={tol:.3e}")
    assert all(v <= tol for v in err.values()), (name, err, tol)
    # ---- the scaled checks: the committed state block by block; z-bar, S and nu of every hypothesis at the scale of S
    K, H = zs.shape[0], got["z_pred"].shape[0]
    idv = np.broadcast_to(np.asarray(ids, dtype=np.int64), (c.n,))
    point = lambda k: pts[k] if hyp else pts   # noqa: E731
    evals = {}

    def f32(k):   # candidate k alone: the all-float32 and the float64 evaluation of its sensor call
        if k not in evals:
            evals[k] = {p: ff.sensor_meas(c.model, c.mu, c.cov, idv, zs[k], c.Q, c.mount, point(k), c.gyro, prec=p) for p in ("f32", "f64")}
        return evals[k]
    if state:
        sel = np.maximum(ref["best"], 0)
        rows = np.arange(c.n)
        zb, pb = zs[sel, rows], (pts[sel, rows] if hyp else pts)
        keep = (ref["best"] < 0) | (ref["status"] != 0)

        def st32():
            both = [ff.sensor_meas(c.model, c.mu, c.cov, idv, zb, c.Q, c.mount, pb, c.gyro, keep=keep, prec=p) for p in ("f32", "f64")]
            return tuple((o["mu"], o["cov"]) for o in both)
        fsp.judge_state("associate/" + name, c.model, c.pname, got["mu"], got["cov"], ref["mu"], ref["cov"], f32=st32)
    dims = np.array([sr.meas_dim(int(i)) if i in sr.ids_of(man_of(c.model)) else 0 for i in idv])
    every = ~np.isnan(ref["maha"]).any(axis=0)
    for m in (1, 3):
        sel = every & (dims == m)
        if not sel.any():
            continue
        for hx in range(H):
            ks = [hx] if hyp else list(range(K))
            pick = lambda o: (o["z_pred"][hx][sel][:, :m], o["S"][hx][sel][:, :m, :m], o["innov"][ks][:, sel][:, :, :m])   # noqa: E731
            one = lambda p: (f32(ks[0])[p]["z_pred"][sel][:, :m], f32(ks[0])[p]["S"][sel][:, :m, :m],   # noqa: E731
                             np.stack([f32(k)[p]["innov"][sel][:, :m] for k in ks]))
            fsp.judge_meas(f"associate/{name}/m={m}/h={hx}", c.pname, *pick(got), *pick(ref), f32=lambda: (one("f32"), one("f64")))


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("hyp", [False, True], ids=["shared", "per-hypothesis"])
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_parity(spe, model, pname, hyp):
    """every model id of the engine (and -1 and an id of the other engine) cycling through the batch, K = 4"""
    c = acase(spe, model, pname)
    ids = cycling_ids(model, c.n)
    zs, pts, truth = constructed(c, ids, K4, hyp)
    ref = reference(c, ids, zs, pts, hyp)
    live = np.isin(ids, sr.ids_of(man_of(model)))
    assert np.array_equal(ref["status"], np.where(live, 0, ST_INACTIVE)) and np.array_equal(ref["best"], np.where(live, truth, -1))
    e = engine_of(spe, c)
    got = run(e, ids, zs, c.Q, c.mount, pts, hyp)
    assert np.array_equal(e.status(), got["status"])   # commit = 1 writes the engine's own status array too
    e.close()
    assert got["z_pred"].shape[0] == (K4 if hyp else 1)
    assert np.array_equal(got["mu"][~live], c.mu[~live]) and np.array_equal(got["cov"][~live], c.cov[~live])
    assert not np.array_equal(got["mu"][live], c.mu[live])
    check_parity(f"{model}/{pname}/{'hyp' if hyp else 'shared'}", c, got, ref, ids, zs, pts, hyp)
    for mid in sr.ids_of(man_of(model)):
        m, rows = sr.meas_dim(mid), ids == mid
        assert (got["z_pred"][:, rows, m:] == 0).all() and (got["innov"][:, rows, m:] == 0).all()
        assert (got["S"][:, rows, m:, :] == 0).all() and (got["S"][:, rows, :, m:] == 0).all()


# ------------------------------------------------------------------------------------------ agreement with the existing call
@pytest.mark.parametrize("hyp", [False, True], ids=["shared", "per-hypothesis"])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_agreement_with_update_sensor_fp64(spe, model, hyp):
    """maha[k], loglik[k] against ukfb_update_sensor_dev(commit = 0) with candidate k; the committed state against
    ukfb_update_sensor_dev(commit = 1) on a twin given z[best] (and b[best]); both within the fp64 tolerance.  The BITS line
    says whether they came out identical (recorded in DESIGN.md 4.26, not asserted)."""
    c = acase(spe, model, "f64")
    ids = cycling_ids(model, c.n)
    zs, pts, truth = constructed(c, ids, K4, hyp)
    e, twin = engine_of(spe, c), engine_of(spe, c)
    got = run(e, ids, zs, c.Q, c.mount, pts, hyp)
    live = np.isin(ids, sr.ids_of(man_of(model)))
    assert np.array_equal(got["best"], np.where(live, truth, -1))
    bits = True
    for k in range(K4):
        one = smc.run(twin, ids, zs[k], c.Q, c.mount, pts[k] if hyp else pts, commit=False)
        hx = k if hyp else 0
        pairs = {"maha": (got["maha"][k], one["maha"]), "loglik": (got["loglik"][k], one["loglik"]), "innov": (got["innov"][k][live], one["innov"][live]),
                 "z_pred": (got["z_pred"][hx], one["z_pred"]), "S": (got["S"][hx], one["S"])}
        for key, (a, b) in pairs.items():
            assert np.array_equal(np.isnan(a), np.isnan(b)), (k, key)
            d = scaled(a[~np.isnan(b)], b[~np.isnan(b)])
            bits = bits and np.array_equal(a, b, equal_nan=True)
            assert d <= c.tol, (k, key, d)
    rows = np.arange(c.n)
    sel = np.maximum(got["best"], 0)
    fin = smc.run(twin, np.where(got["best"] >= 0, ids, -1).astype(np.int32), zs[sel, rows], c.Q, c.mount, pts[sel, rows] if hyp else pts)
    e.close(); twin.close()
    em, ec = scaled(got["mu"], fin["mu"]), scaled(got["cov"], fin["cov"])
    bits_state = np.array_equal(got["mu"], fin["mu"]) and np.array_equal(got["cov"], fin["cov"])
    print(f"PARITY {model}/f64/{'hyp' if hyp else 'shared'}-vs-update_sensor_dev n={c.n} max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e} tol={c.tol:.3e}")
    print(f"BITS {model}/{'hyp' if hyp else 'shared'} scores identical to K read-only sensor calls: {bits}; committed state identical: {bits_state}")
    assert em <= c.tol and ec <= c.tol


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_one_candidate_is_the_sensor_update(spe, model, pname):
    """K = 1 in either mode: every output of ukfb_update_sensor_dev, within tolerance"""
    c = acase(spe, model, pname)
    ids = cycling_ids(model, c.n)
    z = smc.mixed_z(c, ids)
    twin = engine_of(spe, c)
    one = smc.run(twin, ids, z, c.Q, c.mount, c.point)
    twin.close()
    live = np.isin(ids, sr.ids_of(man_of(model)))
    for hyp in (False, True):
        e = engine_of(spe, c)
        got = run(e, ids, z[None], c.Q, c.mount, c.point[None] if hyp else c.point, hyp)
        e.close()
        assert np.array_equal(got["status"], one["status"]) and np.array_equal(got["best"], np.where(live, 0, -1))
        assert np.array_equal(got["n_gated"], live.astype(np.int32))
        err = {k: scaled(got[k], one[k]) for k in ("mu", "cov")}
        for k in FLOATS:
            a, b = got[k][0], one[k]
            assert np.array_equal(np.isnan(a), np.isnan(b)), k
            err[k] = scaled(a[~np.isnan(b)], b[~np.isnan(b)])
        print(f"PARITY {model}/{pname}/K=1/{'hyp' if hyp else 'shared'}-vs-update_sensor_dev " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()))
        assert all(v <= c.tol for v in err.values()), err


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_thirty_two_candidates_and_ties(spe, model):
    """K = 32 on 64 filters, duplicated candidates: the lower index wins, on the device as in the reference"""
    n, K = 64, 32
    c = acase(spe, model, "f64", n)
    mid = sr.POSE_POINT if model == "pose" else sr.ORIENT_NAV_VECTOR
    rng = np.random.default_rng(17)
    for hyp in (False, True):
        zs = c.z[mid][None] + 0.08 * rng.standard_normal((K, n, 3))
        pts = np.broadcast_to(c.point, (K, n, 3)).copy() if hyp else c.point
        zbar = sr.update_sensor(man_of(model), c.mu, c.cov, mid, c.z[mid], c.Q, c.mount, c.point, c.gyro)["z_pred"]
        zs[5] = zs[21] = zbar + 1e-3       # the nearest candidate twice (even filters), a far pair elsewhere
        zs[5, 1::2] = zs[21, 1::2] = zbar[1::2] + 5.0
        zs[30] = zs[9]
        zs[2, ::3] = np.nan
        ref = reference(c, mid, zs, pts, hyp)
        assert (ref["best"][0::2] == 5).all() and not np.isin(ref["best"], (21, 30)).any() and (ref["status"] == 0).all()
        e = engine_of(spe, c)
        got = run(e, mid, zs, c.Q, c.mount, pts, hyp)
        e.close()
        assert np.array_equal(got["maha"][5], got["maha"][21]) and np.array_equal(got["maha"][30], got["maha"][9])
        check_parity(f"{model}/f64/K=32/{'hyp' if hyp else 'shared'}", c, got, ref, mid, zs, pts, hyp)


# -------------------------------------------------------------------------------------------------------------------- gate
@pytest.mark.parametrize("hyp", [False, True], ids=["shared", "per-hypothesis"])
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", ["f64", "f32"])
def test_gate(spe, model, pname, hyp):
    c = acase(spe, model, pname)
    mid = sr.POSE_POINT if model == "pose" else sr.ORIENT_NAV_VECTOR
    zs, pts, truth = constructed(c, mid, K4, hyp)
    free = reference(c, mid, zs, pts, hyp)
    d2 = np.sort(free["maha"], axis=0)
    lo, hi = float(d2[0].max()), float(d2[1].min())
    gate = float(np.sqrt(lo * hi))
    assert 1.1 * lo < gate < hi / 1.1      # at least 10 % away from the true candidates and from the clutter
    e = engine_of(spe, c, gate_chi2=gate)
    got = run(e, mid, zs, c.Q, c.mount, pts, hyp)
    e.close()
    ref = reference(c, mid, zs, pts, hyp, gate=gate)
    assert np.array_equal(got["best"], truth) and (got["n_gated"] == 1).all() and (got["status"] == 0).all()
    check_parity(f"{model}/{pname}/gate/{'hyp' if hyp else 'shared'}", c, got, ref, mid, zs, pts, hyp)
    # a gate below every d^2
    low = 0.5 * float(d2[0].min())
    e = engine_of(spe, c, gate_chi2=low)
    got = run(e, mid, zs, c.Q, c.mount, pts, hyp)
    assert np.array_equal(e.status(), np.full(c.n, ST_REJECTED, dtype=np.uint32))
    e.close()
    assert (got["status"] == ST_REJECTED).all() and (got["best"] == -1).all() and (got["n_gated"] == 0).all()
    assert np.array_equal(got["mu"], c.mu) and np.array_equal(got["cov"], c.cov)
    assert np.isfinite(got["maha"]).all() and np.isfinite(got["loglik"]).all() and np.isfinite(got["z_pred"]).all()
    check_parity(f"{model}/{pname}/gate-below/{'hyp' if hyp else 'shared'}", c, got, reference(c, mid, zs, pts, hyp, gate=low), mid, zs, pts, hyp, state=False)


# ------------------------------------------------------------------------------------------------------- bit-level properties
@pytest.mark.parametrize("hyp", [False, True], ids=["shared", "per-hypothesis"])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_read_only(spe, model, hyp):
    """commit = 0 leaves the whole downloadable engine bit-equal and writes the committing call's outputs"""
    n = 255
    c = acase(spe, model, "f64", n)
    ids = cycling_ids(model, n)
    zs, pts, _ = constructed(c, ids, K4, hyp)

    def fresh():
        e = engine_of(spe, c)
        e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
        return e
    e, twin = fresh(), fresh()
    before = snapshot(e)
    dry = run(e, ids, zs, c.Q, c.mount, pts, hyp, commit=False)
    assert same_snapshot(before, snapshot(e)) and same_snapshot(before, snapshot(twin))
    wet = run(twin, ids, zs, c.Q, c.mount, pts, hyp)
    assert same_candidates(dry, wet, keys=FLOATS + INTS) and np.array_equal(dry["mu"], c.mu) and np.array_equal(dry["cov"], c.cov)
    assert not np.array_equal(wet["mu"], c.mu)
    again = run(e, ids, zs, c.Q, c.mount, pts, hyp)   # commit = 0, then commit = 1: the numbers of commit = 1 alone
    assert same_candidates(again, wet)
    e.close(); twin.close()
    # per-filter Q repeated against ONE 3x3; a device id array filled with one id; the host form
    mid = sr.POSE_POINT if model == "pose" else sr.ORIENT_NAV_VECTOR
    zs, pts, _ = constructed(c, mid, K4, hyp)
    e = fresh()
    base = run(e, mid, zs, c.Q, c.mount, pts, hyp)
    e.close()
    e = fresh()
    assert same_candidates(run(e, np.full(n, mid, dtype=np.int32), zs, c.Q[0], c.mount, pts, hyp, q_uniform=True), base)
    e.close()
    e = fresh()
    o = e.associate_sensor(mid, zs, c.Q, c.mount, pts, point_per_candidate=hyp)
    o["mu"], o["cov"], _ = e.state()
    e.close()
    assert same_candidates(o, base)


@pytest.mark.parametrize("hyp", [False, True], ids=["shared", "per-hypothesis"])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failures_stay_inside_their_filter(spe, model, hyp):
    """an uninitialised filter, a covariance -I, a filter with all-NaN candidates and one whose candidate 0 is NaN, each in a
    wavefront with three healthy filters: with commit = 1 the failing ones keep every bit, the healthy ones have the bits of a
    run without the bad ones"""
    n, dead, neg, all_nan, one_nan = 64, 22, 34, 13, 41
    man = man_of(model)
    e = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    mu, cov, init = e.state()
    assert not init[dead] and init.sum() == n - 1
    mu_f = mu.copy()
    mu_f[dead] = mu[0]
    mount, point, gyro, zt, Q = smc.make_inputs(model, mu_f, np.float64)
    if model == "orient":
        e.set_orient_inputs(gyro=gyro)
    mid = sr.POSE_POINT if model == "pose" else sr.ORIENT_NAV_VECTOR
    zs, pts, truth = ar.constructed_candidates(man, mu_f, cov, mid, zt[mid], Q, mount, point, gyro, K4, hyp)
    clean = run(e, mid, zs, Q, mount, pts, hyp, commit=False)
    assert np.array_equal(clean["status"], np.where(np.arange(n) == dead, ST_UNINIT, 0))
    zb = zs.copy()
    zb[:, all_nan, :] = np.nan
    zb[0, one_nan, 1] = np.nan
    cov_bad = cov.copy()
    cov_bad[neg] = -np.eye(man.D)
    e.initialize(mu[neg:neg + 1], cov_bad[neg:neg + 1], first=neg)
    if model == "orient":
        e.set_orient_inputs(gyro=gyro)
    got = run(e, mid, zb, Q, mount, pts, hyp)
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[neg], expect[all_nan] = ST_UNINIT, ST_CHOLESKY, ST_NONFINITE
    assert np.array_equal(got["status"], expect) and np.array_equal(e.status(), expect)
    failing = expect != 0
    assert np.array_equal(got["mu"][failing], mu[failing], equal_nan=True)
    keep = failing & (np.arange(n) != neg)
    assert np.array_equal(got["cov"][keep], cov[keep], equal_nan=True) and np.array_equal(got["cov"][neg], cov_bad[neg])
    assert all(np.isnan(got[k][:, failing]).all() for k in ("z_pred", "S", "maha", "loglik")) and np.isnan(got["innov"][:, failing, 0]).all()
    assert (got["best"][failing] == -1).all() and (got["n_gated"][failing] == 0).all()
    # the filter whose candidate 0 is absent: NaN there, the others scored; best is the true one or, if that was it, the nearest clutter
    assert np.isnan(got["maha"][0, one_nan]) and np.isfinite(got["maha"][1:, one_nan]).all() and got["n_gated"][one_nan] == K4 - 1
    assert got["best"][one_nan] == (truth[one_nan] if truth[one_nan] != 0 else int(np.nanargmin(got["maha"][:, one_nan])))
    # everyone else: the bits of a clean committing run on a twin
    twin = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    if model == "orient":
        twin.set_orient_inputs(gyro=gyro)
    ok = run(twin, mid, zs, Q, mount, pts, hyp)
    twin.close(); e.close()
    assert same_candidates(ok, clean, keys=FLOATS + INTS)
    healthy = ~failing & (np.arange(n) != one_nan)
    assert same_candidates(got, ok, rows=healthy)
    ref = ar.associate_sensor(man, mu_f, cov_bad, mid, zb, Q, mount, pts, gyro, point_per_candidate=hyp, initialised=init)
    assert np.array_equal(ref["status"], expect) and np.array_equal(ref["best"], got["best"]) and np.array_equal(ref["n_gated"], got["n_gated"])


# ------------------------------------------------------------------------------------------------------------ small batches
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_small_batches(spe, model):
    """1, 2, 3 and 5 filters: one partly filled wavefront, and a full one with a one-row tail"""
    big = acase(spe, model, "f64", 255)
    mid = sr.POSE_RANGE if model == "pose" else sr.ORIENT_NAV_VECTOR
    for n in (1, 2, 3, 5):
        for hyp in (False, True):
            c = smc.Case()
            c.model, c.pname, c.n, c.prec, c.wide, c.tol, c.dtype = model, "f64", n, 0, 0, 1e-9, big.dtype
            c.mu, c.cov, c.mount, c.point, c.gyro, c.Q = big.mu[:n], big.cov[:n], big.mount[:n], big.point[:n], big.gyro[:n], big.Q[:n]
            c.z = {mid: big.z[mid][:n]}
            zs, pts, truth = constructed(c, mid, 3, hyp)
            e = engine_of(spe, c)
            got = run(e, mid, zs, c.Q, c.mount, pts, hyp)
            e.close()
            ref = reference(c, mid, zs, pts, hyp)
            assert (got["status"] == 0).all() and np.array_equal(got["best"], truth)
            check_parity(f"{model}/f64/n={n}/{'hyp' if hyp else 'shared'}", c, got, ref, mid, zs, pts, hyp)


def test_host_array_form_fp32(spe):
    """an fp32 engine: ukfb_associate_sensor narrows the host doubles itself; outputs and state are the bits of the device form
    fed the same values rounded to float32"""
    n = 5
    c = acase(spe, "pose", "f32", n)
    rng = np.random.default_rng(9)
    mid = sr.POSE_POINT
    for hyp in (False, True):
        zs, pts, truth = constructed(c, mid, 3, hyp)
        zs = zs + 1e-3 * rng.standard_normal(zs.shape)          # doubles that are NOT fp32 values
        pts = pts + 1e-3 * rng.standard_normal(pts.shape)
        mount = c.mount + 1e-3 * rng.standard_normal((n, 7))
        assert not np.array_equal(zs, stored(zs, np.float32))
        e, twin = engine_of(spe, c), engine_of(spe, c)
        o = e.associate_sensor(mid, zs, c.Q, mount, pts, point_per_candidate=hyp)
        o["mu"], o["cov"], _ = e.state()
        dev = run(twin, mid, stored(zs, np.float32), c.Q, stored(mount, np.float32), stored(pts, np.float32), hyp)
        assert same_candidates(o, dev) and np.array_equal(e.status(), twin.status()) and (o["status"] == 0).all() and np.array_equal(o["best"], truth)
        e.close(); twin.close()


def test_refused_arguments_write_nothing(spe):
    """a uniform id of the other engine: UKFB_ERR_WRONG_MODEL; 0 and 33 candidates: UKFB_ERR_OUT_OF_RANGE; state and outputs untouched"""
    for model, wrong in (("pose", sr.ORIENT_VELOCITY), ("orient", sr.POSE_POSITION), ("pose", -1), ("orient", 8)):
        c = acase(spe, model, "f64", 255)
        mid = sr.ids_of(man_of(model))[0]
        e = engine_of(spe, c)
        with pytest.raises(spe.UkfbError, match="code 5"):
            run(e, wrong, c.z[mid][None], c.Q, c.mount, c.point)
        assert np.array_equal(e.state()[0], c.mu)
        e.close()
    c = acase(spe, "pose", "f64", 255)
    e = engine_of(spe, c)
    n, dt = c.n, torch.float64
    zd = torch.zeros((33, n, 3), dtype=dt, device="cuda")
    qd = torch.from_numpy(np.ascontiguousarray(c.Q.reshape(n, 9))).to("cuda", dt)
    outs = {k: torch.full(shape, FILL, dtype=dt, device="cuda") for k, shape in
            (("z_pred", (33, n, 3)), ("S", (33, n, 9)), ("innov", (33, n, 3)), ("maha", (33, n)), ("loglik", (33, n)))}
    ints = {k: torch.full((n,), -9, dtype=torch.int32, device="cuda") for k in INTS}
    for K in (0, 33, -1):
        for hyp in (False, True):
            with pytest.raises(spe.UkfbError, match="code 4"):
                e.associate_sensor_dev(sr.POSE_POSITION, K, zd, qd, point_dev=zd if hyp else None, point_per_candidate=hyp, **outs, **ints)
    e.sync()
    torch.cuda.synchronize()
    assert all(bool((v == FILL).all()) for v in outs.values()) and all(bool((v == -9).all()) for v in ints.values())
    assert np.array_equal(e.state()[0], c.mu) and np.array_equal(e.state()[1], c.cov)
    with pytest.raises(spe.UkfbError, match="code 1"):   # per-hypothesis mode without the points
        e.associate_sensor_dev(sr.POSE_POINT, 2, zd, qd, point_per_candidate=True, **outs, **ints)
    e.close()
