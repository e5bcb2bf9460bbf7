"""Probabilistic data association on the device (ukfb_update_pda_dev / ukfb_update_pda, include/ukf_batch_pda.h).

States, inputs, engines, the three precision modes and their tolerances are those of tests/test_gpu_sensor_meas.py
(tests/sensor_meas_cases.py: PRECS, case, engine_of, make_inputs), but for the length of OrientationState's nav-frame vectors
(pcase below, the association test's choice).  Candidates are the constructed inputs of tests/pda_reference.constructed_pda:
prescribed Mahalanobis radii rotated through the candidates, three of four inside the gate of 16, every 7th filter with all
four outside -- and every comparison first asserts pda_reference.conditions on the reference's own numbers (every d^2 5 % clear
of the gate, beta_0 inside (0.01, 0.99) on at least half of the filters with a gated candidate), so that no decision here
hinges on rounding and all three terms of the covariance carry weight.  The reference is tests/pda_reference.py on the state AS
DOWNLOADED and the inputs AS STORED.

Bounds.  best, n_gated, status and the NaN patterns are equal.  fp64 and fp32-wide: |x - ref| <= tol (1 + |ref|) with PRECS'
tol on mean, covariance, z-bar, S, nu, d^2, log-likelihood, beta, beta_0 and nu-bar (wide against the reference rounded to
fp32), and the scaled checks of tests/feature_scaled_parity.py on the state and on z-bar, S, nu.  Plain fp32 has no bound fixed
in advance: the state and z-bar, S, nu are held by judge_state / judge_meas to M_FEAT times the distance of the all-float32 CPU
evaluation of the same call (tests/pda_f32.py) from its float64 twin; d^2, log-likelihood, beta, beta_0 and nu-bar to
max(1e-4, M_FEAT x that evaluation's own distance).  Every distance is printed as a PARITY line before anything asserts; the
maxima measured on an MI355X are in profiles/pda_parity.txt."""
import numpy as np
import pytest
import torch

import feature_scaled_parity as fsp
import pda_f32
import pda_reference as pr
import sensor_meas_cases as smc
import sensor_meas_reference as sr
from engine_support import cycled_engine, man_of, same_snapshot, scaled, snapshot, stored, tdt
from probe_support import LDS_PATTERNS, lds_poison
from sensor_meas_cases import PRECS, case, cycling_ids, engine_of

pytestmark = pytest.mark.gpu

K4 = 4
ST_NONFINITE, ST_CHOLESKY, ST_UNINIT, ST_INACTIVE, ST_REJECTED = 1 << 4, 1 << 5, 1 << 7, 1 << 8, 1 << 9
PER_CANDIDATE = ("innov", "maha", "loglik", "beta")
PER_FILTER = ("z_pred", "S", "beta0", "innov_comb")
FLOATS = PER_FILTER + PER_CANDIDATE
INTS = ("best", "n_gated", "status")
FILL = -7.0
WEIGHTS = ("maha", "loglik", "beta", "beta0", "innov_comb")   # plain fp32: max(1e-4, M_FEAT x the fp32 evaluation's own distance)


def rule_of(spe, r=pr.RULE):
    return spe.PdaRule(*r)


def run(e, ids, z, Q, mount, point, rule=pr.RULE, commit=True, q_uniform=False, poison=None):
    """-> dict(mu, cov, z_pred [n, 3], S [n, 3, 3], innov [K, n, 3], maha, loglik, beta [K, n], beta0 [n], innov_comb [n, 3], best,
    n_gated, status [n]) after update_pda_dev; mount [7] / point [3]: uniform; poison: an LDS pattern planted in front of the call"""
    n, dt, K = e.capacity, tdt(e), int(np.shape(z)[0])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    zd = dev(z)
    qd = dev(np.asarray(Q).reshape(9) if q_uniform else np.asarray(Q).reshape(n, 9))
    idd = None if np.isscalar(ids) else torch.from_numpy(np.asarray(ids, dtype=np.int32)).to("cuda")
    mount, point = np.asarray(mount), np.asarray(point)
    md = dev(mount) if mount.ndim == 2 else None
    pd = dev(point) if point.ndim == 2 else None
    full = lambda shape, v=FILL, t=dt: torch.full(shape, v, dtype=t, device="cuda")   # noqa: E731
    o = {"z_pred": full((n, 3)), "S": full((n, 9)), "innov": full((K, n, 3)), "maha": full((K, n)), "loglik": full((K, n)),
         "beta": full((K, n)), "beta0": full((n,)), "innov_comb": full((n, 3)),
         "best": full((n,), -9, torch.int32), "n_gated": full((n,), -9, torch.int32), "status": full((n,), -1, torch.int32)}
    torch.cuda.synchronize()
    if poison is not None:
        e.sync()
        assert lds_poison()(poison) == 0
    e.update_pda_dev(int(ids) if idd is None else 0, K, zd, qd, rule_of(smc.slam_pose_estimation_amd, rule), q_is_uniform=q_uniform,
                     model_dev=idd, mount_dev=md, mount=mount if md is None else smc.spe_identity(), point_dev=pd,
                     point=point if pd is None else (0.0, 0.0, 0.0), commit=commit, **o)
    e.sync()
    torch.cuda.synchronize()
    r = {k: o[k].double().cpu().numpy() for k in FLOATS}
    r["S"] = r["S"].reshape(n, 3, 3)
    r["best"], r["n_gated"] = o["best"].cpu().numpy(), o["n_gated"].cpu().numpy()
    r["status"] = o["status"].cpu().numpy().astype(np.uint32)
    r["mu"], r["cov"], _ = e.state()
    return r


_PCASE = {}


def pcase(spe, model, pname, n=smc.N):
    """The sensor test's case.  OrientationState: the nav-frame vectors of ORIENT_NAV_VECTOR get the length of catalogue
    entries, 1 ... 3, instead of that file's 15 ... 80 -- the choice of tests/test_gpu_associate.py and for its reason: at
    15 ... 80 the S of that model has condition 500 ... 1700, and a plain fp32 d^2 of 10 ... 100 (the radii here reach 9.8)
    carries the relative error of the fp32 S times that condition."""
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


def reference(c, ids, zs, gate=pr.GATE, rule=pr.RULE, **kw):
    return pr.update_pda(man_of(c.model), c.mu, c.cov, ids, zs, c.Q, c.mount, c.point, c.gyro, rule=rule, gate_chi2=gate, **kw)


def constructed(c, ids, K, **kw):
    """-> z [K, n, 3] for the case's batch, as the engine stores them"""
    z_true = c.z[int(ids)] if np.isscalar(ids) else smc.mixed_z(c, ids)
    return pr.constructed_pda(man_of(c.model), c.mu, c.cov, ids, z_true, c.Q, c.mount, c.point, c.gyro, K, c.dtype, **kw)[0]


def same_outputs(a, b, keys=("mu", "cov") + FLOATS + INTS, rows=None):
    """bit equality; rows: a selection of filters (the second axis of the per-candidate outputs)"""
    rows = slice(None) if rows is None else rows
    part = lambda o, k: o[k][:, rows] if k in PER_CANDIDATE else o[k][rows]   # noqa: E731
    return all(np.array_equal(part(a, k), part(b, k), equal_nan=True) for k in keys)


_REFS = {}


def shared_reference(c, ids_key, ids, zs_key, zs, gate=pr.GATE):
    """the float64 reference of a (case, ids, candidates) used by more than one test: computed once, never changed"""
    key = (c.model, c.pname, c.n, ids_key, zs_key, gate)
    if key not in _REFS:
        _REFS[key] = reference(c, ids, zs, gate)
    return _REFS[key]


def check_parity(name, c, got, ref, ids, zs, rule=pr.RULE, tol=None, state=True):
    tol = c.tol if tol is None else tol
    r = {k: np.asarray(ref[k], dtype=np.float64) for k in ("mu", "cov") + FLOATS}
    if c.wide:   # the engine stores fp32
        r = {k: v.astype(np.float32).astype(np.float64) for k, v in r.items()}
    for k in INTS:
        assert np.array_equal(got[k], ref[k]), (name, k, np.nonzero(got[k] != ref[k])[0][:8])
    for k in FLOATS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(r[k])), (name, k)
    err = {k: scaled(got[k], r[k]) for k in ("mu", "cov")} if state else {}
    err.update({k: scaled(got[k][~np.isnan(r[k])], r[k][~np.isnan(r[k])]) for k in FLOATS})
    plain = c.pname == "f32"
    idv = np.broadcast_to(np.asarray(ids, dtype=np.int64), (c.n,))
    evals = {}

    def f32():   # the all-float32 and the float64 evaluation of the same call, once
        if not evals:
            inside = np.nan_to_num(ref["beta"], nan=0.0) > 0.0
            keep = (ref["n_gated"] == 0) | (ref["status"] != 0)
            for p in ("f32", "f64"):
                evals[p] = pda_f32.pda(c.model, c.mu, c.cov, idv, zs, c.Q, c.mount, c.point, c.gyro, rule, inside, keep=keep, prec=p)
        return evals
    bound = {k: tol for k in err}
    if plain:   # no bound fixed in advance: the weights' from the fp32 evaluation's own distance, the rest from the scaled checks
        own = (ref["status"] & pr.FAILED) == 0
        fin = lambda k, x: x[:, own] if k in PER_CANDIDATE else x[own]   # noqa: E731
        for k in WEIGHTS:
            a, b = fin(k, f32()["f32"][k]), fin(k, f32()["f64"][k])
            d32 = scaled(a[~np.isnan(b)], b[~np.isnan(b)])
            bound[k] = max(1e-4, fsp.M_FEAT * d32)
            print(f"PARITY {name} n={c.n} fp32-evaluation distance d32_{k}={d32:.3e} bound={bound[k]:.3e}")
    print(f"PARITY {name} n={c.n} K={zs.shape[0]} " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={tol:.3e}")
    held = WEIGHTS if plain else tuple(err)
    assert all(err[k] <= bound[k] for k in held), (name, {k: (err[k], bound[k]) for k in held if not err[k] <= bound[k]})
    # ---- the scaled checks: the committed state block by block; z-bar, S and nu at the scale of S
    if state:
        fsp.judge_state("pda/" + name, c.model, c.pname, got["mu"], got["cov"], ref["mu"], ref["cov"],
                        f32=lambda: tuple((f32()[p]["mu"], f32()[p]["cov"]) for p in ("f32", "f64")))
    dims = pr.kernel_dim(man_of(c.model), idv)
    every = ~np.isnan(ref["maha"]).any(axis=0) & np.isin(idv, sr.ids_of(man_of(c.model)))
    for m in (1, 3):
        sel = every & (dims == m)
        if not sel.any():
            continue
        pick = lambda o: (o["z_pred"][sel][:, :m], o["S"][sel][:, :m, :m], o["innov"][:, sel][:, :, :m])   # noqa: E731
        fsp.judge_meas(f"pda/{name}/m={m}", c.pname, *pick(got), *pick(ref), f32=lambda: (pick(f32()["f32"]), pick(f32()["f64"])))


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_parity(spe, model, pname):
    """every model id of the engine (and -1 and an id of the other engine) cycling through the batch, K = 4, commit = 1; the
    all-outside filters: REJECTED_GATE, the state bit for bit, beta_0 = 1 and beta_k = 0 exactly"""
    c = pcase(spe, model, pname)
    ids = cycling_ids(model, c.n)
    zs = constructed(c, ids, K4)
    ref = shared_reference(c, "cycling", ids, "K4", zs)
    share = pr.conditions(ref)
    print(f"PARITY {model}/{pname} share of 0.01 < beta_0 < 0.99 among the filters with a gated candidate: {share:.3f}")
    assert share >= 0.5
    live = np.isin(ids, sr.ids_of(man_of(model)))
    out = live & (np.arange(c.n) % 7 == 6)
    assert np.array_equal(ref["status"], np.where(live, np.where(out, ST_REJECTED, 0), ST_INACTIVE))
    assert (ref["n_gated"][live & ~out] == 3).all()
    e = engine_of(spe, c, gate_chi2=pr.GATE)
    got = run(e, ids, zs, c.Q, c.mount, c.point)
    assert np.array_equal(e.status(), got["status"])   # commit = 1 writes the engine's own status array too
    e.close()
    keep = ~live | out
    assert np.array_equal(got["mu"][keep], c.mu[keep]) and np.array_equal(got["cov"][keep], c.cov[keep])
    assert not np.array_equal(got["mu"][live & ~out], c.mu[live & ~out])
    assert (got["beta0"][out] == 1.0).all() and (got["beta"][:, out] == 0.0).all() and (got["innov_comb"][out] == 0.0).all()
    assert np.isfinite(got["maha"][:, out]).all() and (got["best"][out] == -1).all()
    check_parity(f"{model}/{pname}", c, got, ref, ids, zs)
    for mid in sr.ids_of(man_of(model)):
        m, rows = sr.meas_dim(mid), ids == mid
        assert (got["z_pred"][rows, m:] == 0).all() and (got["innov"][:, rows, m:] == 0).all() and (got["innov_comb"][rows, m:] == 0).all()
        assert (got["S"][rows, m:, :] == 0).all() and (got["S"][rows, :, m:] == 0).all()
    ok = (got["status"] & pr.FAILED) == 0
    total = got["beta0"][ok] + got["beta"][:, ok].sum(axis=0)
    assert np.abs(total - 1.0).max() <= (1e-5 if c.dtype == np.float32 else 1e-12)


@pytest.mark.parametrize("K", [1, 32])
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_one_and_thirty_two_candidates(spe, model, pname, K):
    """K = 32: radii 0.5 + 0.3 k spread across the gate; K = 1: one candidate at radius 1"""
    c = pcase(spe, model, pname, 255)
    ids = cycling_ids(model, c.n)
    zs = constructed(c, ids, K)
    ref = reference(c, ids, zs)
    assert pr.conditions(ref) >= 0.5
    live = np.isin(ids, sr.ids_of(man_of(model)))
    assert (ref["n_gated"][live] == (12 if K == 32 else 1)).all()
    e = engine_of(spe, c, gate_chi2=pr.GATE)
    got = run(e, ids, zs, c.Q, c.mount, c.point)
    e.close()
    check_parity(f"{model}/{pname}/K={K}", c, got, ref, ids, zs)


# ------------------------------------------------------------------------------------------------------------------ limits
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_no_clutter_one_candidate_is_the_sensor_update(spe, model, pname):
    """lambda = 1e-300, K = 1, the gate off: the state of ukfb_update_sensor_dev on a twin within tol; beta_1 == 1 exactly and
    beta_0 < 1e-30"""
    c = pcase(spe, model, pname)
    ids = cycling_ids(model, c.n)
    z = smc.mixed_z(c, ids)
    twin = engine_of(spe, c)
    one = smc.run(twin, ids, z, c.Q, c.mount, c.point)
    twin.close()
    e = engine_of(spe, c)
    got = run(e, ids, z[None], c.Q, c.mount, c.point, rule=pr.RULE._replace(clutter_m1=1e-300, clutter_m3=1e-300))
    e.close()
    live = np.isin(ids, sr.ids_of(man_of(model)))
    assert np.array_equal(got["status"], one["status"]) and np.array_equal(got["best"], np.where(live, 0, -1))
    assert (got["beta"][0][live] == 1.0).all() and (got["beta0"][live] < 1e-30).all() and (got["beta0"][live] >= 0.0).all()
    err = {k: scaled(got[k], one[k]) for k in ("mu", "cov")}
    for k, a in (("z_pred", got["z_pred"]), ("S", got["S"]), ("innov", got["innov"][0]), ("maha", got["maha"][0]), ("loglik", got["loglik"][0]),
                 ("innov_comb", got["innov_comb"])):
        b = one["innov" if k == "innov_comb" else k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        err[k] = scaled(a[~np.isnan(b)], b[~np.isnan(b)])
    bits = np.array_equal(got["mu"], one["mu"]) and np.array_equal(got["cov"], one["cov"])
    print(f"PARITY {model}/{pname}/K=1/no-clutter-vs-update_sensor_dev " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) +
          f" tol={c.tol:.3e}")
    print(f"BITS {model}/{pname} no-clutter K=1 state identical to update_sensor_dev: {bits}")
    assert all(v <= c.tol for v in err.values()), err
    assert not np.array_equal(got["mu"][live], c.mu[live])


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_scores_agree_with_the_association(spe, model, pname):
    """z-bar, S, nu, d^2, log-likelihood, best and n_gated against ukfb_associate_sensor_dev (shared-h, commit = 0) on the same
    inputs, within tol; the BITS line says whether they came out identical (recorded in DESIGN.md, not asserted)"""
    c = pcase(spe, model, pname)
    ids = cycling_ids(model, c.n)
    zs = constructed(c, ids, K4)
    e = engine_of(spe, c, gate_chi2=pr.GATE)
    before = snapshot(e)
    got = run(e, ids, zs, c.Q, c.mount, c.point, commit=False)
    n, dt = c.n, tdt(e)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    full = lambda shape, t=dt: torch.full(shape, FILL, dtype=t, device="cuda")   # noqa: E731
    o = {"z_pred": full((1, n, 3)), "S": full((1, n, 9)), "innov": full((K4, n, 3)), "maha": full((K4, n)), "loglik": full((K4, n)),
         "best": full((n,), torch.int32), "n_gated": full((n,), torch.int32), "status": full((n,), torch.int32)}
    e.associate_sensor_dev(0, K4, dev(zs), dev(c.Q.reshape(n, 9)), model_dev=torch.from_numpy(ids).to("cuda"), mount_dev=dev(c.mount),
                           point_dev=dev(c.point), commit=False, **o)
    e.sync()
    torch.cuda.synchronize()
    assert same_snapshot(before, snapshot(e))
    e.close()
    asc = {k: v.double().cpu().numpy() for k, v in o.items()}
    asc["z_pred"], asc["S"] = asc["z_pred"][0], asc["S"][0].reshape(n, 3, 3)
    assert np.array_equal(got["best"], asc["best"].astype(np.int32)) and np.array_equal(got["n_gated"], asc["n_gated"].astype(np.int32))
    assert np.array_equal(got["status"], asc["status"].astype(np.uint32))
    err, bits = {}, True
    for k in ("z_pred", "S", "innov", "maha", "loglik"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(asc[k])), k
        err[k] = scaled(got[k][~np.isnan(asc[k])], asc[k][~np.isnan(asc[k])])
        bits = bits and np.array_equal(got[k], asc[k], equal_nan=True)
    print(f"PARITY {model}/{pname}/vs-associate_sensor_dev " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={c.tol:.3e}")
    print(f"BITS {model}/{pname} scores identical to associate_sensor_dev (shared-h, commit = 0): {bits}")
    assert all(v <= c.tol for v in err.values()), err


# ------------------------------------------------------------------------------------------------------- bit-level properties
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_permuted_candidates(spe, model, pname):
    """the association's scores permuted bit for bit; the state, the weights (they hold the normaliser, a sum in the candidates'
    order) and nu-bar within tol"""
    c = pcase(spe, model, pname, 255)
    ids = cycling_ids(model, c.n)
    zs = constructed(c, ids, K4)
    perm = np.array([2, 0, 3, 1])
    e, twin = engine_of(spe, c, gate_chi2=pr.GATE), engine_of(spe, c, gate_chi2=pr.GATE)
    a, b = run(e, ids, zs, c.Q, c.mount, c.point), run(twin, ids, zs[perm], c.Q, c.mount, c.point)
    e.close(); twin.close()
    for k in ("innov", "maha", "loglik"):
        assert np.array_equal(a[k][perm], b[k], equal_nan=True), k
    assert same_outputs(a, b, keys=("z_pred", "S", "n_gated", "status"))
    some = a["best"] >= 0
    assert np.array_equal(perm[b["best"][some]], a["best"][some]) and np.array_equal(a["best"] < 0, b["best"] < 0)
    tol = 1e-4 if pname == "f32" else c.tol   # (plain fp32: the tolerance of PRECS; two orders of one fp32 sum)
    err = {k: scaled(np.nan_to_num(x), np.nan_to_num(y)) for k, (x, y) in
           dict(mu=(a["mu"], b["mu"]), cov=(a["cov"], b["cov"]), beta=(a["beta"][perm], b["beta"]), beta0=(a["beta0"], b["beta0"]),
                innov_comb=(a["innov_comb"], b["innov_comb"])).items()}
    assert np.array_equal(np.isnan(a["beta"][perm]), np.isnan(b["beta"]))
    print(f"PARITY {model}/{pname}/permuted " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={tol:.3e}")
    assert all(v <= tol for v in err.values()), err


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_read_only_and_input_forms(spe, model):
    """commit = 0 leaves the whole downloadable engine bit-equal and writes the committing call's outputs; per-filter Q repeated
    against ONE 3 x 3, a device id array against one id, device mount and point against uniform ones, the host form"""
    n = 255
    c = pcase(spe, model, "f64", n)
    ids = cycling_ids(model, n)
    zs = constructed(c, ids, K4)

    def fresh():
        e = engine_of(spe, c, gate_chi2=pr.GATE)
        e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
        return e
    e, twin = fresh(), fresh()
    before = snapshot(e)
    dry = run(e, ids, zs, c.Q, c.mount, c.point, commit=False)
    assert same_snapshot(before, snapshot(e)) and same_snapshot(before, snapshot(twin))
    wet = run(twin, ids, zs, c.Q, c.mount, c.point)
    assert same_outputs(dry, wet, keys=FLOATS + INTS) and np.array_equal(dry["mu"], c.mu) and np.array_equal(dry["cov"], c.cov)
    assert not np.array_equal(wet["mu"], c.mu)
    again = run(e, ids, zs, c.Q, c.mount, c.point)   # commit = 0, then commit = 1: the numbers of commit = 1 alone
    assert same_outputs(again, wet)
    e.close(); twin.close()
    mid = sr.POSE_POINT if model == "pose" else sr.ORIENT_NAV_VECTOR
    mount1, point1 = c.mount[0], c.point[0]
    mountn, pointn = np.broadcast_to(mount1, (n, 7)).copy(), np.broadcast_to(point1, (n, 3)).copy()
    z_true = stored(sr.h(mid, c.mu, mountn, pointn, c.gyro), c.dtype)
    zs = pr.constructed_pda(man_of(model), c.mu, c.cov, mid, z_true, c.Q[0], mount1, point1, c.gyro, K4, c.dtype)[0]
    e = fresh()
    base = run(e, mid, zs, c.Q, mountn, pointn)
    e.close()
    assert (base["status"][np.arange(n) % 7 != 6] == 0).all() and (base["n_gated"][np.arange(n) % 7 != 6] == 3).all()
    e = fresh()
    assert same_outputs(run(e, np.full(n, mid, dtype=np.int32), zs, c.Q[0], mount1, point1, q_uniform=True), base)
    e.close()
    e = fresh()
    o = e.update_pda(mid, zs, c.Q, rule_of(spe), mount1, point1)
    o["mu"], o["cov"], _ = e.state()
    e.close()
    assert same_outputs(o, base)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failures_stay_inside_their_filter(spe, model):
    """an uninitialised filter, a negative id, a NaN in Q, a filter with all-NaN candidates, one whose candidate 1 is NaN and a
    covariance -I, each in a wavefront with healthy filters: with commit = 1 the failing ones keep every bit and get the header's
    status and NaN, the healthy ones have the bits of a run without the failures"""
    n, dead, noid, qnan, all_nan, one_nan, neg = 64, 22, 9, 50, 13, 41, 34
    man = man_of(model)
    e = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,), gate_chi2=pr.GATE)
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
    clean = run(e, ids, zs, Q, mount, point, commit=False)
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
    got = run(e, idb, zb, Qb, mount, point)
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[noid], expect[qnan], expect[all_nan], expect[neg] = ST_UNINIT, ST_INACTIVE, ST_NONFINITE, ST_NONFINITE, ST_CHOLESKY
    assert np.array_equal(got["status"], expect) and np.array_equal(e.status(), expect)
    failing = expect != 0
    assert np.array_equal(got["mu"][failing], mu[failing], equal_nan=True)
    keep = failing & (np.arange(n) != neg)
    assert np.array_equal(got["cov"][keep], cov[keep], equal_nan=True) and np.array_equal(got["cov"][neg], cov_bad[neg])
    assert all(np.isnan(got[k][:, failing]).all() for k in ("maha", "loglik", "beta")) and np.isnan(got["innov"][:, failing, 0]).all()
    assert all(np.isnan(got[k][failing]).all() for k in ("z_pred", "S", "beta0")) and np.isnan(got["innov_comb"][failing, 0]).all()
    assert (got["best"][failing] == -1).all() and (got["n_gated"][failing] == 0).all()
    # the filter whose candidate 1 is absent: NaN there, and the rest act as K - 1 candidates would
    assert np.isnan(got["beta"][1, one_nan]) and np.isnan(got["maha"][1, one_nan]) and np.isfinite(got["maha"][[0, 2, 3], one_nan]).all()
    ref = pr.update_pda(man, mu_f, cov_bad, idb, zb, Qb, mount, point, gyro, gate_chi2=pr.GATE, initialised=init)
    three = pr.update_pda(man, mu_f, cov_bad, idb, zb[[0, 2, 3]], Qb, mount, point, gyro, gate_chi2=pr.GATE, initialised=init)
    assert np.array_equal(ref["status"], expect) and np.array_equal(ref["best"], got["best"]) and np.array_equal(ref["n_gated"], got["n_gated"])
    assert got["n_gated"][one_nan] == three["n_gated"][one_nan]
    for a, b in ((got["mu"][one_nan], three["mu"][one_nan]), (got["cov"][one_nan], three["cov"][one_nan]),
                 (got["beta"][[0, 2, 3], one_nan], three["beta"][:, one_nan]), (got["beta0"][one_nan], three["beta0"][one_nan])):
        assert scaled(np.asarray(a), np.asarray(b)) <= 1e-9
    # everyone else: the bits of a clean committing run on a twin
    twin = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,), gate_chi2=pr.GATE)
    if model == "orient":
        twin.set_orient_inputs(gyro=gyro)
    ok = run(twin, ids, zs, Q, mount, point)
    twin.close(); e.close()
    assert same_outputs(ok, clean, keys=FLOATS + INTS)
    healthy = ~failing & (np.arange(n) != one_nan)
    assert same_outputs(got, ok, rows=healthy)


# ------------------------------------------------------------------------------------------------------------ small batches
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_small_batches(spe, model):
    """1, 2, 3 and 5 filters: one partly filled wavefront, and a full one with a one-row tail"""
    big = pcase(spe, model, "f64", 255)
    mid = sr.POSE_RANGE if model == "pose" else sr.ORIENT_NAV_VECTOR
    for n in (1, 2, 3, 5):
        c = smc.Case()
        c.model, c.pname, c.n, c.prec, c.wide, c.tol, c.dtype = model, "f64", n, 0, 0, 1e-9, big.dtype
        c.mu, c.cov, c.mount, c.point, c.gyro, c.Q = big.mu[:n], big.cov[:n], big.mount[:n], big.point[:n], big.gyro[:n], big.Q[:n]
        c.z = {mid: big.z[mid][:n]}
        zs = constructed(c, mid, K4, all_outside=False)
        e = engine_of(spe, c, gate_chi2=pr.GATE)
        got = run(e, mid, zs, c.Q, c.mount, c.point)
        e.close()
        ref = reference(c, mid, zs)
        assert (got["status"] == 0).all() and (got["n_gated"] == 3).all()
        check_parity(f"{model}/f64/n={n}", c, got, ref, mid, zs)


def test_host_array_form_fp32(spe):
    """an fp32 engine: ukfb_update_pda narrows the host doubles itself; outputs and state are the bits of the device form fed the
    same values rounded to float32"""
    n = 5
    c = pcase(spe, "pose", "f32", n)
    rng = np.random.default_rng(9)
    mid = sr.POSE_POINT
    zs = constructed(c, mid, K4, all_outside=False)
    zs = zs + 1e-3 * rng.standard_normal(zs.shape)          # doubles that are NOT fp32 values
    mount = c.mount + 1e-3 * rng.standard_normal((n, 7))
    point = c.point + 1e-3 * rng.standard_normal((n, 3))
    assert not np.array_equal(zs, stored(zs, np.float32))
    e, twin = engine_of(spe, c, gate_chi2=pr.GATE), engine_of(spe, c, gate_chi2=pr.GATE)
    o = e.update_pda(mid, zs, c.Q, rule_of(spe), mount, point)
    o["mu"], o["cov"], _ = e.state()
    dev = run(twin, mid, stored(zs, np.float32), c.Q, stored(mount, np.float32), stored(point, np.float32))
    assert same_outputs(o, dev) and np.array_equal(e.status(), twin.status()) and (o["status"] == 0).all() and (o["n_gated"] > 0).all()
    e.close(); twin.close()


def test_refused_arguments_write_nothing(spe):
    """every refused argument returns its code and leaves pre-filled outputs and the state untouched"""
    for model, wrong in (("pose", sr.ORIENT_VELOCITY), ("orient", sr.POSE_POSITION), ("pose", -1), ("orient", 8)):
        c = pcase(spe, model, "f64", 255)
        mid = sr.ids_of(man_of(model))[0]
        e = engine_of(spe, c)
        with pytest.raises(spe.UkfbError, match="code 5"):   # UKFB_ERR_WRONG_MODEL
            run(e, wrong, c.z[mid][None], c.Q, c.mount, c.point)
        assert np.array_equal(e.state()[0], c.mu)
        e.close()
    c = pcase(spe, "pose", "f64", 255)
    e = engine_of(spe, c)
    n, dt = c.n, torch.float64
    zd = torch.zeros((33, n, 3), dtype=dt, device="cuda")
    qd = torch.from_numpy(np.ascontiguousarray(c.Q.reshape(n, 9))).to("cuda", dt)
    outs = {k: torch.full(shape, FILL, dtype=dt, device="cuda") for k, shape in
            (("z_pred", (n, 3)), ("S", (n, 9)), ("innov", (33, n, 3)), ("maha", (33, n)), ("loglik", (33, n)), ("beta", (33, n)),
             ("beta0", (n,)), ("innov_comb", (n, 3)))}
    ints = {k: torch.full((n,), -9, dtype=torch.int32, device="cuda") for k in INTS}
    good = pr.RULE
    for K in (0, 33, -1):
        with pytest.raises(spe.UkfbError, match="code 4"):   # UKFB_ERR_OUT_OF_RANGE
            e.update_pda_dev(sr.POSE_POSITION, K, zd, qd, rule_of(spe), **outs, **ints)
    bad_rules = [good._replace(p_detect=0.0), good._replace(p_detect=1.5), good._replace(p_gate_m1=0.0), good._replace(p_gate_m3=float("nan")),
                 good._replace(clutter_m1=0.0), good._replace(clutter_m3=float("inf")), good._replace(clutter_m3=-1.0),
                 good._replace(p_detect=1.0, p_gate_m1=1.0), good._replace(p_detect=1.0, p_gate_m3=1.0)]
    for r in bad_rules:
        with pytest.raises(spe.UkfbError, match="code 1"):   # UKFB_ERR_INVALID_ARG
            e.update_pda_dev(sr.POSE_POSITION, 4, zd, qd, rule_of(spe, r), **outs, **ints)
    # per-hypothesis candidates are refused: the structure of the association with point_per_candidate = 1
    ain = spe.engine.AssociateIn(model_dev=None, candidates=4, z_dev=zd.data_ptr(), Q_dev=qd.data_ptr(), q_is_uniform=0, mount_dev=None,
                                 point_dev=zd.data_ptr(), point_per_candidate=1)
    ain.mount_uniform[6] = 1.0
    out = spe.PdaOut(*[outs[k].data_ptr() for k in ("z_pred", "S", "innov", "maha", "loglik", "beta", "beta0", "innov_comb")],
                     *[ints[k].data_ptr() for k in INTS])
    import ctypes as C
    rule = rule_of(spe)
    assert e._lib.ukfb_update_pda_dev(e._h, sr.POSE_POINT, C.byref(ain), C.byref(rule), 1, C.byref(out)) == 1
    assert e._lib.ukfb_update_pda_dev(e._h, sr.POSE_POINT, C.byref(ain), None, 1, C.byref(out)) == 1
    with pytest.raises(spe.UkfbError, match="code 1"):   # commit = 0 and nothing to compute
        e.update_pda_dev(sr.POSE_POSITION, 4, zd, qd, rule_of(spe), commit=False)
    e.sync()
    torch.cuda.synchronize()
    assert all(bool((v == FILL).all()) for v in outs.values()) and all(bool((v == -9).all()) for v in ints.values())
    assert np.array_equal(e.state()[0], c.mu) and np.array_equal(e.state()[1], c.cov)
    e.close()


# ------------------------------------------------------------------------------------------------------------ LDS leftovers
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_lds_leftovers_do_not_reach_the_result(spe, model, pname):
    """the LDS of every compute unit filled with a NaN pattern and with all ones right in front of the launch: the bits of the
    run that found whatever the test before left there"""
    c = pcase(spe, model, pname, 255)
    ids = cycling_ids(model, c.n)
    zs = constructed(c, ids, K4)
    runs = []
    for pat in (None, LDS_PATTERNS[0], LDS_PATTERNS[2]):
        e = engine_of(spe, c, gate_chi2=pr.GATE)
        runs.append(run(e, ids, zs, c.Q, c.mount, c.point, poison=pat))
        e.close()
    assert same_outputs(runs[1], runs[0]) and same_outputs(runs[2], runs[0])
    assert (runs[0]["status"][np.isin(ids, sr.ids_of(man_of(model)))] & pr.FAILED == 0).all()
