"""The sensor-frame update with given association weights on the device (ukfb_update_weighted_dev / ukfb_update_weighted,
include/ukf_batch_jpda.h), and the whole chain update_pda_dev(commit = 0) -> jpda_scenes_dev -> update_weighted_dev.

States, inputs, engines, the three precision modes and their tolerances are those of tests/test_gpu_pda.py
(tests/sensor_meas_cases.py: PRECS, case, engine_of; OrientationState's nav-frame vectors at the length of catalogue entries,
pcase below), candidates the constructed inputs of tests/pda_reference.constructed_pda.  The reference is
tests/jpda_reference.update_weighted on the state AS DOWNLOADED and the inputs AS STORED.

Bounds.  n_used, status and the NaN patterns are equal.  fp64 and fp32-wide: |x - ref| <= tol (1 + |ref|) with PRECS' tol on
mean, covariance, z-bar, S, nu, d^2, log-likelihood, weight_used, beta_0 and nu-bar (wide against the reference rounded to
fp32), and the scaled checks of tests/feature_scaled_parity.py on the state and on z-bar, S, nu.  Plain fp32 has no bound fixed
in advance: the state and z-bar, S, nu are held by judge_state / judge_meas to M_FEAT times the distance of the all-float32 CPU
evaluation of the same call (tests/jpda_f32.py) from its float64 twin; d^2, log-likelihood, weight_used, beta_0 and nu-bar to
max(1e-4, M_FEAT x that evaluation's own distance).  Every distance is printed as a PARITY line before anything asserts; the
maxima measured on an MI355X are in profiles/jpda_parity.txt."""
import numpy as np
import pytest
import torch

import feature_scaled_parity as fsp
import jpda_f32
import jpda_reference as jr
import pda_reference as pr
import sensor_meas_cases as smc
import sensor_meas_reference as sr
from engine_support import cycled_engine, man_of, same_snapshot, scaled, snapshot, stored, tdt
from oracle import ukf_numpy as on
from probe_support import LDS_PATTERNS, lds_poison
from sensor_meas_cases import PRECS, case, cycling_ids, engine_of

pytestmark = pytest.mark.gpu

K4 = 4
ST_NONFINITE, ST_CHOLESKY, ST_UNINIT, ST_INACTIVE, ST_REJECTED = 1 << 4, 1 << 5, 1 << 7, 1 << 8, 1 << 9
PER_CANDIDATE = ("innov", "maha", "loglik", "weight_used")
PER_FILTER = ("z_pred", "S", "beta0", "innov_comb")
FLOATS = PER_FILTER + PER_CANDIDATE
INTS = ("n_used", "status")
FILL = -7.0
WEIGHTS = ("maha", "loglik", "weight_used", "beta0", "innov_comb")   # plain fp32: max(1e-4, M_FEAT x the fp32 evaluation's own distance)
WEIGHT_SETS = ("below", "one", "above", "odd", "zero")


def run(e, ids, z, Q, mount, point, weight, commit=True, poison=None):
    """-> dict(mu, cov, z_pred [n, 3], S [n, 3, 3], innov [K, n, 3], maha, loglik, weight_used [K, n], beta0 [n], innov_comb [n, 3],
    n_used, status [n]) after update_weighted_dev; weight [K, n] as the engine stores it, or a device tensor; mount [7] / point
    [3]: uniform; poison: an LDS pattern planted in front of the call"""
    n, dt, K = e.capacity, tdt(e), int(np.shape(z)[0])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    zd = dev(z)
    qd = dev(np.asarray(Q).reshape(n, 9))
    wd = weight if torch.is_tensor(weight) else dev(weight)
    idd = None if np.isscalar(ids) else torch.from_numpy(np.asarray(ids, dtype=np.int32)).to("cuda")
    mount, point = np.asarray(mount), np.asarray(point)
    md = dev(mount) if mount.ndim == 2 else None
    pd = dev(point) if point.ndim == 2 else None
    full = lambda shape, v=FILL, t=dt: torch.full(shape, v, dtype=t, device="cuda")   # noqa: E731
    o = {"z_pred": full((n, 3)), "S": full((n, 9)), "innov": full((K, n, 3)), "maha": full((K, n)), "loglik": full((K, n)),
         "weight_used": full((K, n)), "beta0": full((n,)), "innov_comb": full((n, 3)),
         "n_used": full((n,), -9, torch.int32), "status": full((n,), -1, torch.int32)}
    torch.cuda.synchronize()
    if poison is not None:
        e.sync()
        assert lds_poison()(poison) == 0
    e.update_weighted_dev(int(ids) if idd is None else 0, K, zd, qd, wd, model_dev=idd, mount_dev=md,
                          mount=mount if md is None else smc.spe_identity(), point_dev=pd, point=point if pd is None else (0.0, 0.0, 0.0),
                          commit=commit, **o)
    e.sync()
    torch.cuda.synchronize()
    r = {k: o[k].double().cpu().numpy() for k in FLOATS}
    r["S"] = r["S"].reshape(n, 3, 3)
    r["n_used"] = o["n_used"].cpu().numpy()
    r["status"] = o["status"].cpu().numpy().astype(np.uint32)
    r["mu"], r["cov"], _ = e.state()
    return r


_PCASE = {}


def pcase(spe, model, pname, n=smc.N):
    """The sensor test's case; OrientationState: the nav-frame vectors at the length of catalogue entries, 1 ... 3 (the choice
    of tests/test_gpu_pda.py, for its reason: the conditioning of S in plain fp32)"""
    c0 = case(spe, model, pname, n)
    if model == "pose":
        return c0
    key = (pname, n)
    if key not in _PCASE:
        c = smc.Case()
        c.__dict__.update(c0.__dict__)
        rng = np.random.default_rng(29)
        c.point = stored(c0.point / np.linalg.norm(c0.point, axis=1, keepdims=True) * rng.uniform(1.0, 3.0, (n, 1)), c.dtype)
        c.z = dict(c0.z)
        mid = sr.ORIENT_NAV_VECTOR
        c.z[mid] = stored(sr.h(mid, c.mu, c.mount, c.point, c.gyro) + 0.05 * rng.standard_normal((n, 3)), c.dtype)
        c.refs = {}
        _PCASE[key] = c
    return _PCASE[key]


def constructed(c, ids, K, **kw):
    """-> z [K, n, 3] for the case's batch, as the engine stores them"""
    z_true = c.z[int(ids)] if np.isscalar(ids) else smc.mixed_z(c, ids)
    return pr.constructed_pda(man_of(c.model), c.mu, c.cov, ids, z_true, c.Q, c.mount, c.point, c.gyro, K, c.dtype, **kw)[0]


def weights_of(kind, K, n, dtype, seed=37):
    """the weight sets, as an engine of `dtype` stores them: sums below 1, exactly 1 (dyadic), above 1, with NaN, negative and
    zero entries, all zero"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.05, 0.2, size=(K, n))
    if kind == "one":
        w = np.broadcast_to(np.array([0.5, 0.25, 0.125, 0.125])[(np.arange(K)[:, None] + np.arange(n)[None, :]) % K], (K, n)).copy()
    elif kind == "above":
        w = 8.0 * w   # every sum is at least 8 x 4 x 0.05 = 1.6
    elif kind == "odd":
        w[0, ::2], w[1, ::3], w[2, ::5], w[3, 1::4] = np.nan, -0.3, 0.0, np.inf
    elif kind == "zero":
        w = np.zeros((K, n))
    return w.astype(dtype).astype(np.float64)


def reference(c, ids, zs, w, **kw):
    return jr.update_weighted(man_of(c.model), c.mu, c.cov, ids, zs, c.Q, c.mount, c.point, w, c.gyro, **kw)


def same_outputs(a, b, keys=("mu", "cov") + FLOATS + INTS, rows=None):
    """bit equality; rows: a selection of filters (the second axis of the per-candidate outputs)"""
    rows = slice(None) if rows is None else rows
    part = lambda o, k: o[k][:, rows] if k in PER_CANDIDATE else o[k][rows]   # noqa: E731
    return all(np.array_equal(part(a, k), part(b, k), equal_nan=True) for k in keys)


def check_parity(name, c, got, ref, ids, zs, w, tol=None):
    tol = c.tol if tol is None else tol
    r = {k: np.asarray(ref[k], dtype=np.float64) for k in ("mu", "cov") + FLOATS}
    if c.wide:   # the engine stores fp32
        r = {k: v.astype(np.float32).astype(np.float64) for k, v in r.items()}
    for k in INTS:
        assert np.array_equal(got[k], ref[k]), (name, k, np.nonzero(got[k] != ref[k])[0][:8])
    for k in FLOATS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(r[k])), (name, k)
    err = {k: scaled(got[k], r[k]) for k in ("mu", "cov")}
    err.update({k: scaled(got[k][~np.isnan(r[k])], r[k][~np.isnan(r[k])]) for k in FLOATS})
    plain = c.pname == "f32"
    idv = np.broadcast_to(np.asarray(ids, dtype=np.int64), (c.n,))
    evals = {}

    def f32():   # the all-float32 and the float64 evaluation of the same call, once
        if not evals:
            used = np.nan_to_num(ref["weight_used"], nan=0.0) > 0.0
            keep = (ref["n_used"] == 0) | (ref["status"] != 0)
            for p in ("f32", "f64"):
                evals[p] = jpda_f32.weighted(c.model, c.mu, c.cov, idv, zs, c.Q, c.mount, c.point, c.gyro, w, used, keep=keep, prec=p)
        return evals
    bound = {k: tol for k in err}
    if plain:   # no bound fixed in advance: the weights' from the fp32 evaluation's own distance, the rest from the scaled checks
        own = (ref["status"] & jr.FAILED) == 0
        fin = lambda k, x: x[:, own] if k in PER_CANDIDATE else x[own]   # noqa: E731
        for k in WEIGHTS:
            a, b = fin(k, f32()["f32"][k]), fin(k, f32()["f64"][k])
            d32 = scaled(a[~np.isnan(b)], b[~np.isnan(b)])
            bound[k] = max(1e-4, fsp.M_FEAT * d32)
            print(f"PARITY weighted/{name} n={c.n} fp32-evaluation distance d32_{k}={d32:.3e} bound={bound[k]:.3e}")
    print(f"PARITY weighted/{name} n={c.n} K={zs.shape[0]} " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={tol:.3e}")
    held = WEIGHTS if plain else tuple(err)
    assert all(err[k] <= bound[k] for k in held), (name, {k: (err[k], bound[k]) for k in held if not err[k] <= bound[k]})
    fsp.judge_state("weighted/" + name, c.model, c.pname, got["mu"], got["cov"], ref["mu"], ref["cov"],
                    f32=lambda: tuple((f32()[p]["mu"], f32()[p]["cov"]) for p in ("f32", "f64")))
    dims = pr.kernel_dim(man_of(c.model), idv)
    every = ~np.isnan(ref["maha"]).any(axis=0) & np.isin(idv, sr.ids_of(man_of(c.model)))
    for m in (1, 3):
        sel = every & (dims == m)
        if not sel.any():
            continue
        pick = lambda o: (o["z_pred"][sel][:, :m], o["S"][sel][:, :m, :m], o["innov"][:, sel][:, :, :m])   # noqa: E731
        fsp.judge_meas(f"weighted/{name}/m={m}", c.pname, *pick(got), *pick(ref), f32=lambda: (pick(f32()["f32"]), pick(f32()["f64"])))


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_parity(spe, model, pname, kind):
    """every model id of the engine (and -1 and an id of the other engine) cycling through the batch, K = 4, commit = 1, one
    weight set per case.  All zero: REJECTED_GATE, the state bit for bit, beta_0 = 1 and nu-bar = 0 exactly"""
    c = pcase(spe, model, pname)
    ids = cycling_ids(model, c.n)
    zs = constructed(c, ids, K4)
    w = weights_of(kind, K4, c.n, c.dtype)
    ref = reference(c, ids, zs, w)
    live = np.isin(ids, sr.ids_of(man_of(model)))
    e = engine_of(spe, c, gate_chi2=1e-3)   # such a gate would reject everything, if the gate played a part
    got = run(e, ids, zs, c.Q, c.mount, c.point, w)
    assert np.array_equal(e.status(), got["status"])   # commit = 1 writes the engine's own status array too
    e.close()
    assert np.array_equal(got["mu"][~live], c.mu[~live]) and np.array_equal(got["cov"][~live], c.cov[~live])
    if kind == "zero":
        assert np.array_equal(ref["status"], np.where(live, ST_REJECTED, ST_INACTIVE)) and np.array_equal(got["status"], ref["status"])
        assert np.array_equal(got["mu"], c.mu) and np.array_equal(got["cov"], c.cov)
        assert (got["beta0"][live] == 1.0).all() and (got["weight_used"][:, live] == 0.0).all() and (got["innov_comb"][live] == 0.0).all()
        assert np.isfinite(got["maha"][:, live]).all() and (got["n_used"] == 0).all()
    else:
        assert np.array_equal(ref["status"], np.where(live, 0, ST_INACTIVE))
        assert not np.array_equal(got["mu"][live], c.mu[live])
        s = got["weight_used"][:, live].sum(axis=0) + got["beta0"][live]
        assert np.abs(s - 1.0).max() <= (1e-5 if c.dtype == np.float32 else 1e-12)
        if kind in ("one", "above"):
            assert np.abs(got["beta0"][live]).max() <= (1e-6 if c.dtype == np.float32 else 1e-15)
        if kind == "odd":
            assert (got["n_used"][live] >= 1).all() and (got["n_used"][live] < K4).any()
    check_parity(f"{model}/{pname}/{kind}", c, got, ref, ids, zs, w)


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_pdas_own_weights_commit_pdas_state(spe, model, pname):
    """with the beta that update_pda_dev(commit = 0) wrote (a device buffer, handed on as it is), update_weighted_dev commits
    the state of update_pda_dev(commit = 1) on a twin engine, within the tolerances of the parity test, with equal status words"""
    c = pcase(spe, model, pname)
    ids = cycling_ids(model, c.n)
    zs = constructed(c, ids, K4)
    dt = torch.float64 if c.dtype == np.float64 else torch.float32
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    rule = spe.PdaRule(*pr.RULE)
    args = dict(model_dev=torch.from_numpy(ids).to("cuda"), mount_dev=dev(c.mount), point_dev=dev(c.point))
    e, twin = engine_of(spe, c, gate_chi2=pr.GATE), engine_of(spe, c, gate_chi2=pr.GATE)
    beta = torch.full((K4, c.n), FILL, dtype=dt, device="cuda")
    st_dry = torch.full((c.n,), -1, dtype=torch.int32, device="cuda")
    st_pda = torch.full((c.n,), -1, dtype=torch.int32, device="cuda")
    before = snapshot(e)
    e.update_pda_dev(0, K4, dev(zs), dev(c.Q.reshape(c.n, 9)), rule, commit=False, beta=beta, status=st_dry, **args)
    e.sync()
    assert same_snapshot(before, snapshot(e))
    got = run(e, ids, zs, c.Q, c.mount, c.point, beta)
    twin.update_pda_dev(0, K4, dev(zs), dev(c.Q.reshape(c.n, 9)), rule, commit=True, status=st_pda, **args)
    twin.sync()
    mu_p, cov_p, _ = twin.state()
    assert np.array_equal(got["status"], st_pda.cpu().numpy().astype(np.uint32)) and np.array_equal(e.status(), twin.status())
    assert np.array_equal(st_dry.cpu().numpy(), st_pda.cpu().numpy())
    e.close(); twin.close()
    out = (got["status"] & ST_REJECTED) != 0
    assert np.array_equal(got["mu"][out], c.mu[out]) and np.array_equal(got["cov"][out], c.cov[out])
    em, ec = scaled(got["mu"], mu_p), scaled(got["cov"], cov_p)
    tol = 1e-4 if pname == "f32" else c.tol   # (plain fp32: the tolerance of PRECS; the weights crossed memory as fp32 once)
    bits = np.array_equal(got["mu"], mu_p) and np.array_equal(got["cov"], cov_p)
    print(f"PARITY weighted/{model}/{pname}/pda-weights-vs-update_pda_dev max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e} tol={tol:.3e}")
    print(f"BITS weighted/{model}/{pname} state identical to update_pda_dev(commit = 1): {bits}")
    assert em <= tol and ec <= tol
    assert not np.array_equal(got["mu"], c.mu)


# ------------------------------------------------------------------------------------------------------- bit-level properties
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_read_only_and_the_host_form(spe, model):
    """commit = 0 leaves the whole downloadable engine bit-equal and writes the committing call's outputs; the host-array form
    gives the bits of the device form"""
    n = 255
    c = pcase(spe, model, "f64", n)
    ids = cycling_ids(model, n)
    zs = constructed(c, ids, K4)
    w = weights_of("below", K4, n, c.dtype)

    def fresh():
        e = engine_of(spe, c)
        e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
        return e
    e, twin = fresh(), fresh()
    before = snapshot(e)
    dry = run(e, ids, zs, c.Q, c.mount, c.point, w, commit=False)
    assert same_snapshot(before, snapshot(e)) and same_snapshot(before, snapshot(twin))
    wet = run(twin, ids, zs, c.Q, c.mount, c.point, w)
    assert same_outputs(dry, wet, keys=FLOATS + INTS) and np.array_equal(dry["mu"], c.mu) and np.array_equal(dry["cov"], c.cov)
    assert not np.array_equal(wet["mu"], c.mu)
    again = run(e, ids, zs, c.Q, c.mount, c.point, w)   # commit = 0, then commit = 1: the numbers of commit = 1 alone
    assert same_outputs(again, wet)
    e.close(); twin.close()
    e = fresh()
    o = e.update_weighted(ids, zs, c.Q, w, c.mount, c.point)
    o["mu"], o["cov"], _ = e.state()
    e.close()
    assert same_outputs(o, wet)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failures_stay_inside_their_filter(spe, model):
    """an uninitialised filter, a negative id, a NaN in Q, a filter with all-NaN candidates, one whose candidate 1 is NaN and a
    covariance -I, each in a wavefront with healthy filters: with commit = 1 the failing ones keep every bit and get the header's
    status and NaN, the healthy ones have the bits of a run without the failures"""
    n, dead, noid, qnan, all_nan, one_nan, neg = 64, 22, 9, 50, 13, 41, 34
    man = man_of(model)
    e = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    mu, cov, init = e.state()
    assert not init[dead] and init.sum() == n - 1
    mu_f = mu.copy()
    mu_f[dead] = mu[0]
    mount, point, gyro, zt, Q = smc.make_inputs(model, mu_f, np.float64)
    if model == "orient":
        e.set_orient_inputs(gyro=gyro)
    mid = sr.POSE_POINT if model == "pose" else sr.ORIENT_SPECIFIC_FORCE
    ids = np.full(n, mid, dtype=np.int32)
    zs = pr.constructed_pda(man, mu_f, cov, ids, zt[mid], Q, mount, point, gyro, K4, all_outside=False)[0]
    w = weights_of("below", K4, n, np.float64)
    clean = run(e, ids, zs, Q, mount, point, w, commit=False)
    assert np.array_equal(clean["status"], np.where(np.arange(n) == dead, ST_UNINIT, 0))
    idb, zb, Qb = ids.copy(), zs.copy(), Q.copy()
    idb[noid] = -1
    Qb[qnan, 1, 1] = np.nan
    zb[:, all_nan, :] = np.nan
    zb[1, one_nan, 1] = np.nan
    cov_bad = cov.copy()
    cov_bad[neg] = -np.eye(man.D)
    e.initialize(mu[neg:neg + 1], cov_bad[neg:neg + 1], first=neg)
    if model == "orient":
        e.set_orient_inputs(gyro=gyro)
    got = run(e, idb, zb, Qb, mount, point, w)
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[noid], expect[qnan], expect[all_nan], expect[neg] = ST_UNINIT, ST_INACTIVE, ST_NONFINITE, ST_NONFINITE, ST_CHOLESKY
    assert np.array_equal(got["status"], expect) and np.array_equal(e.status(), expect)
    failing = expect != 0
    assert np.array_equal(got["mu"][failing], mu[failing], equal_nan=True)
    keep = failing & (np.arange(n) != neg)
    assert np.array_equal(got["cov"][keep], cov[keep], equal_nan=True) and np.array_equal(got["cov"][neg], cov_bad[neg])
    assert all(np.isnan(got[k][:, failing]).all() for k in ("maha", "loglik", "weight_used")) and np.isnan(got["innov"][:, failing, 0]).all()
    assert all(np.isnan(got[k][failing]).all() for k in ("z_pred", "S", "beta0")) and np.isnan(got["innov_comb"][failing, 0]).all()
    assert (got["n_used"][failing] == 0).all()
    # the filter whose candidate 1 is absent: NaN there, and its weight does not count
    assert np.isnan(got["weight_used"][1, one_nan]) and np.isnan(got["maha"][1, one_nan]) and got["n_used"][one_nan] == 3
    ref = jr.update_weighted(man, mu_f, cov_bad, idb, zb, Qb, mount, point, w, gyro, initialised=init)
    assert np.array_equal(ref["status"], expect) and np.array_equal(ref["n_used"], got["n_used"])
    for k in ("mu", "cov", "beta0"):
        assert scaled(got[k][one_nan], ref[k][one_nan]) <= 1e-9, k
    # everyone else: the bits of a clean committing run on a twin
    twin = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    if model == "orient":
        twin.set_orient_inputs(gyro=gyro)
    ok = run(twin, ids, zs, Q, mount, point, w)
    twin.close(); e.close()
    assert same_outputs(ok, clean, keys=FLOATS + INTS)
    healthy = ~failing & (np.arange(n) != one_nan)
    assert same_outputs(got, ok, rows=healthy)


def test_refused_arguments_write_nothing(spe):
    c = pcase(spe, "pose", "f64", 255)
    e = engine_of(spe, c)
    n, dt = c.n, torch.float64
    zd = torch.zeros((33, n, 3), dtype=dt, device="cuda")
    qd = torch.from_numpy(np.ascontiguousarray(c.Q.reshape(n, 9))).to("cuda", dt)
    wd = torch.full((33, n), 0.1, dtype=dt, device="cuda")
    st = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    b0 = torch.full((n,), FILL, dtype=dt, device="cuda")
    for K in (0, 33, -1):
        with pytest.raises(spe.UkfbError, match="code 4"):   # UKFB_ERR_OUT_OF_RANGE
            e.update_weighted_dev(sr.POSE_POSITION, K, zd, qd, wd, status=st, beta0=b0)
    with pytest.raises(spe.UkfbError, match="code 5"):       # UKFB_ERR_WRONG_MODEL
        e.update_weighted_dev(sr.ORIENT_VELOCITY, 4, zd, qd, wd, status=st, beta0=b0)
    with pytest.raises(spe.UkfbError, match="code 1"):       # no weights
        e.update_weighted_dev(sr.POSE_POSITION, 4, zd, qd, None, status=st, beta0=b0)
    with pytest.raises(spe.UkfbError, match="code 1"):       # commit = 0 and nothing to compute
        e.update_weighted_dev(sr.POSE_POSITION, 4, zd, qd, wd, commit=False)
    import ctypes as C
    ain = spe.engine.AssociateIn(model_dev=None, candidates=4, z_dev=zd.data_ptr(), Q_dev=qd.data_ptr(), q_is_uniform=0, mount_dev=None,
                                 point_dev=zd.data_ptr(), point_per_candidate=1)
    ain.mount_uniform[6] = 1.0
    assert e._lib.ukfb_update_weighted_dev(e._h, sr.POSE_POINT, C.byref(ain), wd.data_ptr(), 1, None) == 1   # per-hypothesis candidates
    e.sync()
    torch.cuda.synchronize()
    assert bool((st == -9).all()) and bool((b0 == FILL).all())
    assert np.array_equal(e.state()[0], c.mu) and np.array_equal(e.state()[1], c.cov)
    e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_lds_leftovers_do_not_reach_the_result(spe, model, pname):
    """the LDS of every compute unit filled with a NaN pattern and with all ones right in front of the launch: the bits of the
    run that found whatever the test before left there"""
    c = pcase(spe, model, pname, 255)
    ids = cycling_ids(model, c.n)
    zs = constructed(c, ids, K4)
    w = weights_of("odd", K4, c.n, c.dtype)
    runs = []
    for pat in (None, LDS_PATTERNS[0], LDS_PATTERNS[2]):
        e = engine_of(spe, c)
        runs.append(run(e, ids, zs, c.Q, c.mount, c.point, w, poison=pat))
        e.close()
    assert same_outputs(runs[1], runs[0]) and same_outputs(runs[2], runs[0])
    assert (runs[0]["status"][np.isin(ids, sr.ids_of(man_of(model)))] & jr.FAILED == 0).all()


# -------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name,prec,tol", [("f64", 0, 1e-9), ("f32", 1, 1e-4)], ids=["f64", "f32"])
def test_end_to_end(spe, name, prec, tol):
    """update_pda_dev(commit = 0) -> jpda_scenes_dev into the same beta and beta0 -> update_weighted_dev on the constructed
    scenes (tests/jpda_reference.end_to_end_case: neighbours 1.5 sigma apart, so that they share detections), against the
    reference chain on the state as downloaded.  The joint weights within the bounds of tests/test_gpu_jpda.py around the
    reference's on ITS scores, widened by what the device's scores differ (the PDA test's tolerance on loglik moves beta by at
    most that much: d beta / d l <= 1/4 per pair); the committed state within the tolerance of the sensor-frame family.  Plain
    fp32, as in the parity test: max(1e-4, M_FEAT x the distance of the all-float32 CPU chain from its float64 twin)."""
    mu0, cov0 = spe.synth.pose_initial(smc.N)
    c = jr.end_to_end_case(mu0, cov0)
    n, K, starts = smc.N, jr.E2E_K, c["starts"]
    e = spe.BatchPoseUKF(n, precision=prec, gate_chi2=jr.E2E_GATE)
    e.initialize(c["mu"], c["cov"])
    mu, cov, _ = e.state()
    dt = tdt(e)
    st = lambda x: stored(x, e.dtype)   # noqa: E731
    Qs, zs = st(c["Q"]), st(c["z_point"])
    pda, beta_ref, beta0_ref, upd, j = jr.reference_chain(on.POSE, mu, cov, zs, Qs, starts, dtype=e.dtype)
    share = jr.share_of_scenes_that_differ(pda, beta_ref, starts)
    assert share >= 0.5 and (upd["status"] == 0).all()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    z_t, Q_t = dev(c["z_point"]), dev(c["Q"].reshape(n, 9))
    full = lambda shape, t=dt: torch.full(shape, FILL, dtype=t, device="cuda")   # noqa: E731
    maha, loglik, beta, beta0 = full((K, n)), full((K, n)), full((K, n)), full((n,))
    status = full((n,), torch.int32)
    scene_status = full((len(starts) - 1,), torch.int32)
    rule = spe.PdaRule(*jr.E2E_RULE)
    before = snapshot(e, noise_of=(0,))
    torch.cuda.synchronize()
    e.update_pda_dev(sr.POSE_POINT, K, z_t, Q_t, rule, commit=False, maha=maha, loglik=loglik, beta=beta, beta0=beta0)
    e.sync()
    beta_pda = beta.double().cpu().numpy()
    e.jpda_scenes_dev(K, loglik, rule, len(starts) - 1, scene_start_dev=torch.from_numpy(starts).cuda(), maha_dev=maha, gate=jr.E2E_GATE,
                      model=sr.POSE_POINT, beta=beta, beta0=beta0, scene_status=scene_status)
    e.sync()
    assert same_snapshot(before, snapshot(e, noise_of=(0,)))   # nothing so far has touched the filters
    e.update_weighted_dev(sr.POSE_POINT, K, z_t, Q_t, beta, status=status)
    e.sync()
    assert (scene_status.cpu().numpy() == 0).all() and (status.cpu().numpy() == 0).all() and (e.status() == 0).all()
    got_beta, got_beta0 = beta.double().cpu().numpy(), beta0.double().cpu().numpy()
    assert np.array_equal(np.isnan(got_beta), np.isnan(beta_ref)) and np.array_equal(got_beta == 0.0, beta_ref == 0.0)
    eb, eb0 = float(np.nanmax(np.abs(got_beta - beta_ref))), float(np.abs(got_beta0 - beta0_ref).max())
    moved = float(np.nanmax(np.abs(got_beta - beta_pda)))
    mu2, cov2, _ = e.state()
    em, ec = scaled(mu2, upd["mu"]), scaled(cov2, upd["cov"])
    bound = {k: tol for k in ("beta", "beta0", "mu", "cov")}
    if prec:   # plain fp32, as in the parity test: M_FEAT times the distance of the all-float32 CPU chain from its float64 twin
        import pda_f32
        inside = np.nan_to_num(pda["beta"], nan=0.0) > 0.0
        ch = {}
        for p in ("f32", "f64"):
            o = pda_f32.pda("pose", mu, cov, sr.POSE_POINT, zs, Qs, sr.IDENTITY_MOUNT, np.zeros(3), None, jr.E2E_RULE, inside, prec=p)
            jj = jr.jpda_scenes(on.POSE, o["loglik"], o["maha"], starts, sr.POSE_POINT, jr.E2E_RULE, jr.E2E_GATE, np.float32 if p == "f32" else np.float64)
            b = st(jj["beta"]) if p == "f32" else jj["beta"]
            u = jpda_f32.weighted("pose", mu, cov, sr.POSE_POINT, zs, Qs, sr.IDENTITY_MOUNT, np.zeros(3), None, b, np.nan_to_num(b) > 0.0, prec=p)
            ch[p] = {"beta": np.nan_to_num(b), "beta0": jj["beta0"], "mu": u["mu"], "cov": u["cov"]}
        for k in bound:
            d32 = scaled(ch["f32"][k], ch["f64"][k])
            bound[k] = max(tol, fsp.M_FEAT * d32)
            print(f"PARITY jpda/end-to-end/{name} fp32-evaluation distance d32_{k}={d32:.3e} bound={bound[k]:.3e}")
    print(f"PARITY jpda/end-to-end/{name} scenes={len(starts) - 1} share with |beta_JPDA - beta_PDA| >= 0.05: {share:.3f} "
          f"max|beta_JPDA - beta_PDA| on the device={moved:.3f} max_dbeta={eb:.3e} max_dbeta0={eb0:.3e} "
          f"max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e} tol={tol:.3e}")
    assert moved >= 0.05
    assert eb <= bound["beta"] and eb0 <= bound["beta0"] and em <= bound["mu"] and ec <= bound["cov"]
    assert not np.array_equal(mu2, mu)
    e.close()
