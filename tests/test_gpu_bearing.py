"""Bearing measurements on the device (ukfb_update_bearing_dev / ukfb_update_bearing, include/ukf_batch.h).

States as downloaded, inputs (seed 5, tests/bearing_reference.make_inputs) as stored in the engine's precision: mounts
r ~ U(-1, 1)^3, qs = exp(U(-1, 1)^3); z = unit(h(mu) + 0.01 N(0, 1)) U(0.5, 2), so that the normalisation is exercised;
Q = 0.01^2 (I + 0.3 A A^T) per filter, dense.  Three batches per model:
  ordinary  synth.pose_initial / orient_initial after two real cycles, points 15 ... 80 m away;
  tight     the same with Sigma x 1e-8: the theta -> 0 branches of the sphere logarithm;
  wide      the initial states uncycled with Sigma x 4 (Pose; points 0.6 ... 2.0 m from the body origin) / Sigma x 100
            (OrientationState; the scale chosen on the CPU: 762 / 260 of 1022 filters take one / two mean trips, the largest
            sigma-point angle from z-bar is 0.51 rad).  On the Pose batch the reference makes 1 / 2 / 3 / 5 mean trips for
            917 / 97 / 7 / 1 filters and the largest angle is 2.33 rad.  The tests assert from the reference, before they
            compare, that at least 5 % of the filters take two trips or more and that no angle exceeds 2.8 rad.
The reference is tests/bearing_reference.py (the 2 x 2 basis form, pinned by tests/test_bearing_reference.py; the kernel works
in the 3-dimensional embedded form) run on the state AS DOWNLOADED and the inputs AS STORED.  Parity bound:
|x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64) / 1e-4 (fp32) / 1e-9 + 2^-23 (fp32 engines with wide_arithmetic, against the
reference's outputs rounded to fp32), on mean, covariance, z-bar, S, nu, d^2 and log-likelihood.  Every comparison prints a
PARITY line with its maxima before it asserts.  Plain fp32 is held on the ordinary batch only.

Every parity comparison also makes the SCALED ones of tests/feature_scaled_parity.py (imported, not edited): the updated state
whitened by the reference's own sigmas block by block, and z-bar, S, nu -- here all three scaled by s = sqrt(trace(S_ref) / 2)
in every component, since a diagonal entry of the rank-2 S can vanish (v = 1 for S, |nu_i| / s, 1 / s for z-bar).  Bounds:
fp64 1e-9; wide 2 u v + 1e-9; plain fp32 max(M_feat d_32, 20 u v) with d_32 from tests/bearing_f32.py."""
import numpy as np
import pytest
import torch

import bearing_f32 as bf
import bearing_reference as br
import feature_scaled_parity as fsp
from engine_support import ACC_COV, Case, engine_of, man_of, new_engine, same, same_snapshot, scaled, snapshot, tdt
from oracle import ukf_numpy as on

pytestmark = pytest.mark.gpu

N = 1022   # not a multiple of four: the last workgroup holds two filters
PRECS = [("f64", 0, 0, 1e-9), ("f32", 1, 0, 1e-4), ("f32w", 1, 1, 1e-9 + 2.0 ** -23)]
ST_NONFINITE, ST_CHOLESKY, ST_NOCONV, ST_UNINIT, ST_INACTIVE, ST_REJECTED = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8, 1 << 9
OUT_KEYS = ("z_pred", "S", "innov", "maha", "loglik")
ALL_KEYS = ("mu", "cov") + OUT_KEYS + ("status",)
IDENTITY = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
BATCHES = {"ordinary": (True, 1.0, 15.0, 80.0), "tight": (True, 1e-8, 15.0, 80.0), "wide": (False, None, 0.6, 2.0)}
WIDE_SCALE = {"pose": 4.0, "orient": 100.0}


def ids_of(model):
    return br.POSE_IDS if model == "pose" else br.ORIENT_IDS


def main_id(model):
    return br.POSE_POINT if model == "pose" else br.ORIENT_NAV_DIRECTION


def downloaded_state(spe, model, n, prec, wide, cycles, scale):
    """-> (mu, cov, dtype) of an engine initialised from synth's states, after `cycles` real cycles (Pose:
    acceleration branch, POS3; OrientationState: its body-velocity update), the covariance scaled and stored once more"""
    sy = spe.synth
    e = new_engine(spe, model, n, prec, wide)
    mu0, cov0 = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
    e.initialize(mu0, cov0)
    for c in range(cycles):
        mu_now = e.state(with_cov=False)[0]
        if model == "pose":
            acc, z, Q = sy.pose_cycle_inputs(n, c, mu_now[:, :3])
            e.set_acceleration(acc, ACC_COV)
            e.cycle(0.01, spe.MEAS_POS3, z, Q)
        else:
            gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu_now[:, 0:4])
            e.set_orient_inputs(gyro, acc)
            e.cycle(0.01, spe.MEAS_ORIENT_BODYVEL3, z, Q)
    mu, cov, _ = e.state()
    if scale != 1.0:
        e.initialize(mu, scale * cov)
        mu, cov, _ = e.state()
    dtype = e.dtype
    e.close()
    return mu, cov, dtype


_CACHE = {}


def case(spe, model, pname, batch="ordinary", n=N):
    key = (model, pname, batch, n)
    if key not in _CACHE:
        _, prec, wide, tol = [p for p in PRECS if p[0] == pname][0]
        cycled, scale, lo, hi = BATCHES[batch]
        c = Case()
        c.model, c.pname, c.batch, c.n, c.prec, c.wide, c.tol = model, pname, batch, n, prec, wide, tol
        c.mu, c.cov, c.dtype = downloaded_state(spe, model, n, prec, wide, 2 if cycled else 0, WIDE_SCALE[model] if scale is None else scale)
        c.mount, c.point, c.z, c.Q = br.make_inputs(man_of(model), c.mu, lo, hi, c.dtype)
        if model == "pose":
            dist = np.linalg.norm(c.point - c.mu[:, 0:3], axis=1)
            assert lo - 0.01 < dist.min() and dist.max() < hi + 0.01
        c.refs = {}
        _CACHE[key] = c
    return _CACHE[key]


def sub_case(big, n):
    c = Case()
    c.__dict__.update(big.__dict__)
    c.n, c.mu, c.cov, c.mount, c.point, c.Q = n, big.mu[:n], big.cov[:n], big.mount[:n], big.point[:n], big.Q[:n]
    c.z = {k: v[:n] for k, v in big.z.items()}
    c.refs = {}
    return c


def run(e, ids, z, Q, mount, point, commit=True, q_uniform=False):
    """-> dict(mu, cov, z_pred, S, innov, maha, loglik, status) after update_bearing_dev; mount [7] / point [3]: uniform"""
    n, dt = e.capacity, tdt(e)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    zd = dev(z)
    qd = dev(np.asarray(Q).reshape(9) if q_uniform else np.asarray(Q).reshape(n, 9))
    idd = None if np.isscalar(ids) else torch.from_numpy(np.asarray(ids, dtype=np.int32)).to("cuda")
    mount, point = np.asarray(mount), np.asarray(point)
    md = dev(mount) if mount.ndim == 2 else None
    pd = dev(point) if point.ndim == 2 else None
    o = {"z_pred": torch.full((n, 3), -7.0, dtype=dt, device="cuda"), "S": torch.full((n, 9), -7.0, dtype=dt, device="cuda"),
         "innov": torch.full((n, 3), -7.0, dtype=dt, device="cuda"), "maha": torch.full((n,), -7.0, dtype=dt, device="cuda"),
         "loglik": torch.full((n,), -7.0, dtype=dt, device="cuda"), "status": torch.full((n,), -1, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    e.update_bearing_dev(int(ids) if idd is None else 0, zd, qd, q_is_uniform=q_uniform, model_dev=idd, mount_dev=md,
                         mount=mount if md is None else IDENTITY, point_dev=pd, point=point if pd is None else (0.0, 0.0, 0.0),
                         commit=commit, **o)
    e.sync()
    torch.cuda.synchronize()
    r = {k: v.double().cpu().numpy() for k, v in o.items() if k != "status"}
    r["S"] = r["S"].reshape(n, 3, 3)
    r["status"] = o["status"].cpu().numpy().astype(np.uint32)
    r["mu"], r["cov"], _ = e.state()
    return r


def mixed_z(c, ids):
    z = np.ones((c.n, 3))
    for mid in ids_of(c.model):
        z[ids == mid] = c.z[mid][ids == mid]
    return z


def z_of(c, ids):
    return c.z[int(ids)] if np.isscalar(ids) else mixed_z(c, ids)


def run_case(e, c, ids, **kw):
    return run(e, ids, z_of(c, ids), c.Q, c.mount, c.point, **kw)


def reference(c, ids, gate=-1.0, max_it=on.MEAN_MAX_IT):
    key = (int(ids), gate, max_it) if np.isscalar(ids) else None
    if key is not None and key in c.refs:
        return c.refs[key]
    ref = br.update_bearing(man_of(c.model), c.mu, c.cov, ids, z_of(c, ids), c.Q, c.mount, c.point, gate_chi2=gate, max_it=max_it)
    if key is not None:
        c.refs[key] = ref
    return ref


def meas_distances(o, ref):
    """z-bar, S, nu against the reference's, every component at the scale s = sqrt(trace(S_ref) / 2) -> (distances, v)"""
    s = np.sqrt(np.einsum("nii->n", ref["S"]) / 2.0)
    d = {"z_pred": np.abs(o["z_pred"] - ref["z_pred"]) / s[:, None], "S": np.abs(o["S"] - ref["S"]) / (s * s)[:, None, None],
         "nu": np.abs(o["innov"] - ref["innov"]) / s[:, None]}
    v = {"z_pred": np.maximum(1.0, np.abs(ref["z_pred"])) / s[:, None], "S": np.ones(ref["S"].shape), "nu": np.abs(ref["innov"]) / s[:, None]}
    return d, v


def judge_meas(name, mode, got, ref, sel, f32=None):
    """fsp.judge_meas with the bearing's scale: fsp.meas_bound on the distances above"""
    mode = fsp.MODE[mode]
    pick = lambda o: {k: o[k][sel] for k in ("z_pred", "S", "innov")}   # noqa: E731
    d, v = meas_distances(pick(got), pick(ref))
    d_32 = None
    if mode == "f32":
        a, b = f32()
        d_32 = {k: float(x.max()) for k, x in meas_distances(pick(a), pick(b))[0].items()}
    bound = fsp.meas_bound(mode, v, d_32)
    rows = []
    for k in ("z_pred", "S", "nu"):
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(d[k] == 0.0, 0.0, d[k] / bound[k])   # a NaN distance stays NaN and fails below
        at = np.unravel_index(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
        rows.append((k, float(d[k][at]), float(bound[k][at])))
    fsp._line(name, mode, "measurement", rows)
    bad = [(k, dist, bnd) for k, dist, bnd in rows if not dist <= bnd]
    assert not bad, f"{name} [{mode}]: " + "; ".join(f"output {k}: {x:.3e} > bound {t:.3e}" for k, x, t in bad)


def check_parity(name, c, got, ref, ids, rows=None):
    """the file's bound on every output, then the scaled checks: the updated state block by block, and z-bar, S, nu at the scale
    of S; ids: the call's model id(s), for the fp32 evaluation behind a plain fp32 engine's bound"""
    rows = np.ones(c.n, bool) if rows is None else rows
    r = {k: np.asarray(ref[k], dtype=np.float64) for k in ALL_KEYS[:-1]}
    if c.wide:   # the engine stores fp32
        r = {k: v.astype(np.float32).astype(np.float64) for k, v in r.items()}
    scored = rows & ~np.isnan(r["maha"])
    assert np.array_equal(np.isnan(got["maha"][rows]), np.isnan(r["maha"][rows])), name
    err = {k: scaled(got[k][rows], r[k][rows]) for k in ("mu", "cov")}
    err.update({k: scaled(got[k][scored], r[k][scored]) for k in OUT_KEYS})
    print(f"PARITY {name} n={int(rows.sum())} " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={c.tol:.3e}")
    assert all(v <= c.tol for v in err.values()), (name, err, c.tol)
    # what the outputs are, whatever the reference says: a unit vector, a rank-2 S, an innovation in the tangent plane
    u = 2.0 ** -24 if c.prec else 2.0 ** -53
    zb = got["z_pred"][scored]
    assert np.abs(np.sum(zb * zb, axis=1) - 1.0).max() <= 8 * u
    sc = np.sqrt(np.einsum("nii->n", r["S"][scored]) / 2.0)
    assert (np.abs(np.einsum("nij,nj->ni", got["S"][scored], zb)) <= 64 * u * (sc * sc)[:, None] + c.tol * (sc * sc)[:, None]).all()
    assert (np.abs(np.sum(got["innov"][scored] * zb, axis=1)) <= 8 * u * (1.0 + np.linalg.norm(got["innov"][scored], axis=1))).all()
    idv = np.broadcast_to(np.asarray(ids, dtype=np.int64), (c.n,))
    evals = {}

    def f32():
        if not evals:
            for p in ("f32", "f64"):
                evals[p] = bf.update_bearing(c.model, c.mu, c.cov, idv, z_of(c, ids), c.Q, c.mount, c.point, keep=ref["status"] != 0, prec=p)
        return evals
    fsp.judge_state("bearing/" + name, c.model, c.pname, got["mu"][rows], got["cov"][rows], ref["mu"][rows], ref["cov"][rows],
                    f32=lambda: tuple((f32()[p]["mu"][rows], f32()[p]["cov"][rows]) for p in ("f32", "f64")))
    if scored.any():
        judge_meas("bearing/" + name, c.pname, got, ref, scored, f32=lambda: (f32()["f32"], f32()["f64"]))


def cycling_ids(model, n):
    """every model of the engine, -1, an id of the other engine and one beyond 2, so that four wave-mates always differ"""
    table = list(ids_of(model)) + [-1, br.ORIENT_NAV_DIRECTION if model == "pose" else br.POSE_POINT, 3, main_id(model), 7]
    return np.array(table, dtype=np.int32)[np.arange(n) % len(table)]


def assert_wide(ref):
    """the wide batch does what it is there for, by the reference: the mean really iterates, and no sigma point comes near the
    antipode of z-bar"""
    assert (ref["trips"] >= 2).mean() >= 0.05, np.bincount(ref["trips"])
    assert ref["spread"].max() <= 2.8, ref["spread"].max()


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,batch", [("f64", "ordinary"), ("f32", "ordinary"), ("f32w", "ordinary"), ("f64", "tight"),
                                         ("f32w", "tight"), ("f64", "wide"), ("f32w", "wide")])
def test_parity(spe, model, pname, batch):
    c = case(spe, model, pname, batch)
    uniform = {}
    for mid in ids_of(model):
        ref = reference(c, mid)
        assert (ref["status"] == 0).all(), (mid, np.unique(ref["status"]))
        if batch == "wide" and mid == main_id(model):
            assert_wide(ref)
        e = engine_of(spe, c)
        got = run_case(e, c, mid)
        e.close()
        assert (got["status"] == 0).all(), (mid, np.unique(got["status"]))
        check_parity(f"{model}/{pname}/{batch}/{br.NAMES[mid]}", c, got, ref, mid)
        assert not np.array_equal(got["mu"], c.mu)
        uniform[mid] = got
    # per-filter ids, every wavefront mixed: the bits of the uniform runs filter by filter
    per = cycling_ids(model, c.n)
    e = engine_of(spe, c)
    got = run_case(e, c, per)
    assert np.array_equal(e.status(), got["status"])   # commit = 1 writes the engine's own status array too
    e.close()
    idle = ~np.isin(per, ids_of(model))
    assert idle.sum() >= c.n // 3
    assert np.array_equal(got["status"], np.where(idle, ST_INACTIVE, 0))
    assert np.array_equal(got["mu"][idle], c.mu[idle]) and np.array_equal(got["cov"][idle], c.cov[idle])
    assert all(np.isnan(got[k][idle]).all() for k in OUT_KEYS)
    for mid in ids_of(model):
        assert same(got, uniform[mid], ALL_KEYS, rows=per == mid), mid
    check_parity(f"{model}/{pname}/{batch}/per-filter-ids", c, got, reference(c, per), per)


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", ["f64", "f32"])
def test_gate(spe, model, pname):
    """gate_chi2 = the reference's median d^2: accepted and REJECTED_GATE split as the reference's"""
    c = case(spe, model, pname)
    mid = main_id(model)
    free = reference(c, mid)
    gate = float(np.median(free["maha"]))
    assert free["maha"].min() < gate < free["maha"].max()
    ref = reference(c, mid, gate=gate)
    e = engine_of(spe, c, gate_chi2=gate)
    got = run_case(e, c, mid)
    e.close()
    near = np.abs(free["maha"] - gate) <= c.tol * (1.0 + free["maha"])
    print(f"GATE {model}/{pname} gate={gate:.6g} left out {int(near.sum())} of {c.n}")
    assert near.sum() <= c.n // 100, int(near.sum())
    rows = ~near
    assert np.array_equal(got["status"][rows], ref["status"][rows])
    rej = rows & (ref["status"] == ST_REJECTED)
    assert rej.sum() > c.n // 4 and (rows & (ref["status"] == 0)).sum() > c.n // 4
    assert np.array_equal(got["mu"][rej], c.mu[rej]) and np.array_equal(got["cov"][rej], c.cov[rej])
    assert np.isfinite(got["maha"][rej]).all()
    check_parity(f"{model}/{pname}/gate", c, got, ref, mid, rows=rows)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_mean_cap(spe, model):
    """mean_max_iter = 2 on the wide batch, fp64: WARN_MEAN_NOCONV where the reference says so, on every filter whose
    reference step norms all differ from mean_tol by more than 1e-3 relative; the update still commits"""
    c = case(spe, model, "f64", "wide")
    mid = main_id(model)
    ref = reference(c, mid, max_it=2)
    assert_wide(reference(c, mid))
    assert set(np.unique(ref["status"])) == {0, ST_NOCONV}
    clear = ref["tol_margin"] > 1e-3
    print(f"MEANCAP {model} capped {int((ref['status'] == ST_NOCONV).sum())} of {c.n}, left out {int((~clear).sum())}")
    assert (~clear).sum() <= c.n // 100
    e = engine_of(spe, c, mean_max_iter=2)
    got = run_case(e, c, mid)
    e.close()
    assert np.array_equal(got["status"][clear], ref["status"][clear])
    assert (ref["status"][clear] == ST_NOCONV).mean() >= 0.05
    check_parity(f"{model}/f64/wide/mean_max_iter=2", c, got, ref, mid, rows=clear)
    assert not np.array_equal(got["mu"][clear], c.mu[clear])


# ------------------------------------------------------------------------------------------------------- bit-level properties
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_bit_level_properties(spe, model):
    n = 255
    c = sub_case(case(spe, model, "f64"), n)
    per = cycling_ids(model, n)
    mid = main_id(model)
    mount1, point1 = c.mount[7], c.point[7]

    def fresh(**kw):
        e = engine_of(spe, c, **kw)
        e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
        if model == "orient":
            gyro, acc, _, _ = spe.synth.orient_cycle_inputs(n, 0, c.mu[:, 0:4])
            e.set_orient_inputs(gyro, acc)
        return e

    e = fresh()
    base = run(e, mid, c.z[mid], c.Q, mount1, point1)
    e.close()
    assert (base["status"] == 0).all()
    # per-filter mount / point arrays that repeat the uniform ones; a device array filled with the id; per-filter Q repeated
    # against ONE 3x3
    e = fresh()
    assert same(run(e, np.full(n, mid, dtype=np.int32), c.z[mid], c.Q, np.tile(mount1, (n, 1)), np.tile(point1, (n, 1))), base, ALL_KEYS)
    e.close()
    e, e2 = fresh(), fresh()
    assert same(run(e, mid, c.z[mid], c.Q[0], mount1, point1, q_uniform=True),
                run(e2, mid, c.z[mid], np.tile(c.Q[0], (n, 1, 1)), mount1, point1), ALL_KEYS)
    e.close(); e2.close()
    # only the lower triangle of Q is read
    e = fresh()
    Qu = c.Q.copy()
    Qu[:, 0, 1], Qu[:, 0, 2], Qu[:, 1, 2] = 5.0, -3.0, 1e6
    assert same(run(e, mid, c.z[mid], Qu, mount1, point1), base, ALL_KEYS)
    e.close()
    # a gate nothing reaches = no gate
    e = fresh(gate_chi2=1e300)
    assert same(run(e, mid, c.z[mid], c.Q, mount1, point1), base, ALL_KEYS)
    e.close()
    # the host form = the device form (per-filter ids, mounts and points too)
    e = fresh()
    o = e.update_bearing(mid, c.z[mid], c.Q, mount1, point1)
    o["mu"], o["cov"], _ = e.state()
    assert same(o, base, ALL_KEYS)
    e.close()
    e, e2 = fresh(), fresh()
    o = e.update_bearing(per, mixed_z(c, per), c.Q, c.mount, c.point)
    o["mu"], o["cov"], _ = e.state()
    assert same(o, run_case(e2, c, per), ALL_KEYS)
    e.close(); e2.close()
    # commit = 0: the whole downloadable engine keeps its bits, the outputs are the committing call's, and the next
    # prediction is an untouched twin's
    e, twin = fresh(), fresh()
    before = snapshot(e)
    dry = run(e, mid, c.z[mid], c.Q, mount1, point1, commit=False)
    dry_per = run_case(e, c, per, commit=False)
    assert same_snapshot(before, snapshot(e)) and same_snapshot(before, snapshot(twin))
    assert same(dry, base, OUT_KEYS + ("status",)) and np.array_equal(dry["mu"], c.mu) and np.array_equal(dry["cov"], c.cov)
    assert np.array_equal(dry_per["status"], np.where(np.isin(per, ids_of(model)), 0, ST_INACTIVE))
    e.predict(0.013); twin.predict(0.013)
    assert same_snapshot(snapshot(e), snapshot(twin))
    e.close(); twin.close()
    # commit = 0, then commit = 1: the same numbers as commit = 1 alone
    e = fresh()
    run(e, mid, c.z[mid], c.Q, mount1, point1, commit=False)
    assert same(run(e, mid, c.z[mid], c.Q, mount1, point1), base, ALL_KEYS)
    e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_small_batches(spe, model):
    """1, 2, 3 and 5 filters: one partly filled wavefront, and a full one with a one-row tail"""
    big = case(spe, model, "f64", "wide")
    for n in (1, 2, 3, 5):
        c = sub_case(big, n)
        for mid in ids_of(model):
            e = engine_of(spe, c)
            got = run_case(e, c, mid)
            e.close()
            ref = reference(c, mid)
            assert (got["status"] == 0).all() and (ref["status"] == 0).all()
            check_parity(f"{model}/f64/wide/{br.NAMES[mid]}/n={n}", c, got, ref, mid)


@pytest.mark.parametrize("pname", ["f32", "f32w"])
def test_host_array_form_fp32(spe, pname):
    """fp32 engines: ukfb_update_bearing narrows the host doubles itself; its outputs and the committed state are the bits of
    the device form fed the same values rounded to float32.  Five filters."""
    n = 5
    c = sub_case(case(spe, "pose", pname), n)
    rng = np.random.default_rng(9)
    mid = br.POSE_POINT
    f32 = lambda x: np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)   # noqa: E731
    z = c.z[mid] + 1e-3 * rng.standard_normal((n, 3))          # doubles that are NOT fp32 values
    mount = c.mount + 1e-3 * rng.standard_normal((n, 7))
    point = c.point + 1e-3 * rng.standard_normal((n, 3))
    assert not np.array_equal(z, f32(z))
    for mt, pt in ((mount, point), (mount[2], point[2])):
        e, twin = engine_of(spe, c), engine_of(spe, c)
        o = e.update_bearing(mid, z, c.Q, mt, pt)
        o["mu"], o["cov"], _ = e.state()
        dev = run(twin, mid, f32(z), c.Q, f32(mt), f32(pt))
        assert same(o, dev, ALL_KEYS) and np.array_equal(e.status(), twin.status()) and (o["status"] == 0).all()
        e.close(); twin.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failures_stay_inside_their_filter(spe, model):
    """An uninitialised filter, a non-finite and a zero z, a landmark exactly at the mean sensor position (OrientationState:
    b = 0) -- ERR_CHOLESKY -- and Sigma = -I: each sits in a wavefront with three healthy wave-mates, which end with the bits
    of a run without it; NaN in the lever arm of a model that does not read it changes nothing"""
    n, dead = 64, 22
    nan_z, zero_z, at_sensor, neg, unused = 13, 17, 25, 34, 41   # every one in another wavefront
    man = man_of(model)
    sy = spe.synth

    def build():
        e = new_engine(spe, model, n, 0, 0)
        mu0, cov0 = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
        for i in range(n):
            if i != dead:
                e.initialize(mu0[i:i + 1], cov0[i:i + 1], first=i)
        return e
    e = build()
    mu, cov, init = e.state()
    assert not init[dead] and init.sum() == n - 1
    mu_f = mu.copy()
    mu_f[dead] = mu[0]   # (the dead filter's inputs are made from a neighbour's state: they are never used)
    mount, point, zs, Q = br.make_inputs(man, mu_f, 15.0, 80.0)
    ids = np.full(n, main_id(model), dtype=np.int32)
    if model == "pose":
        ids[unused] = br.POSE_NAV_DIRECTION
    z = np.ones((n, 3))
    for mid in ids_of(model):
        z[ids == mid] = zs[mid][ids == mid]
    clean = run(e, ids, z, Q, mount, point, commit=False)
    assert np.array_equal(clean["status"], np.where(np.arange(n) == dead, ST_UNINIT, 0))
    zb, mb, pb = z.copy(), mount.copy(), point.copy()
    zb[nan_z, 1] = np.inf
    zb[zero_z] = 0.0
    if model == "pose":
        mb[at_sensor, 0:3] = 0.0
        pb[at_sensor] = mu[at_sensor, 0:3]   # b - p = 0 at the centre sigma point, exactly
        mb[unused, 0:3] = np.nan             # POSE_NAV_DIRECTION does not read r
    else:
        pb[at_sensor] = 0.0
    cov_bad = cov.copy()
    cov_bad[neg] = -np.eye(man.D)
    e.initialize(mu[neg:neg + 1], cov_bad[neg:neg + 1], first=neg)
    got = run(e, ids, zb, Q, mb, pb)
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[[at_sensor, neg]] = ST_UNINIT, ST_CHOLESKY
    expect[[nan_z, zero_z]] = ST_NONFINITE
    assert np.array_equal(got["status"], expect), (got["status"], expect)
    assert np.array_equal(e.status(), expect)
    failing = expect != 0
    assert np.array_equal(got["mu"][failing], mu[failing], equal_nan=True)
    keep = failing & (np.arange(n) != neg)
    assert np.array_equal(got["cov"][keep], cov[keep], equal_nan=True) and np.array_equal(got["cov"][neg], cov_bad[neg])
    assert all(np.isnan(got[k][failing]).all() for k in OUT_KEYS)
    # everyone else, the filter with NaN in an unused entry included: the bits of a clean committing run on a twin
    twin = build()
    ok = run(twin, ids, z, Q, mount, point)
    twin.close(); e.close()
    assert same(ok, clean, OUT_KEYS + ("status",))
    assert same(got, ok, ALL_KEYS, rows=~failing)
    for i in (at_sensor - 1, at_sensor + 1, unused):
        assert not np.array_equal(got["mu"][i], mu[i])
    ref = br.update_bearing(man, mu_f, cov_bad, ids, zb, Q, mb, pb, initialised=init)
    assert np.array_equal(ref["status"], expect)


def test_uniform_id_of_the_other_engine_is_refused(spe):
    for model, wrong in (("pose", br.ORIENT_NAV_DIRECTION), ("orient", br.POSE_POINT), ("orient", br.POSE_NAV_DIRECTION), ("pose", -1),
                         ("orient", 3)):
        c = sub_case(case(spe, model, "f64"), 255)
        e = engine_of(spe, c)
        with pytest.raises(spe.UkfbError, match="code 5"):
            run(e, wrong, c.z[ids_of(model)[0]], c.Q, c.mount, c.point)
        assert np.array_equal(e.state()[0], c.mu)
        e.close()
