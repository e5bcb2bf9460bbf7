"""The robust sensor-frame update on the device (ukfb_update_robust_dev / ukfb_update_robust, include/ukf_batch_robust.h).

States and inputs: sensor_meas_cases.case -- the state of a cycled engine AS DOWNLOADED, the inputs AS STORED -- with the
innovation of filter i replaced by Ls u rho, rho = (0.5, 1.5, 4, 8, 30, 300)[i mod 6] (robust_reference.contaminate): inliers,
outliers of 0 ... 8 Newton steps and, with the gate at 400, rejected samples side by side in every wavefront.  The reference is
tests/robust_reference.py (pinned by tests/test_robust_reference.py): update_sensor at lambda = 1, lambda by the kernel's rule
restated, update_sensor with lambda Q.  The rule's values reach the kernel rounded to the engine's storage, so the reference
gets them rounded too.  tol of the rule: 1e-13 (fp64, wide_arithmetic), 2e-6 (fp32); max_iter 16.

Bounds.  fp64 and wide_arithmetic: the file's parity bound of tests/test_gpu_sensor_meas.py, |x - ref| <= tol (1 + |ref|) with tol
= 1e-9 / 1e-9 + 2^-23, on lambda, d0^2, d^2, the log-likelihood, z-bar, S, nu and the state.  The residual
|d^2_fp64(lambda_gpu) - c^2| / c^2 of a MATCH row, recomputed by the reference from the GPU's lambda, is held to the same tol:
the row stopped at tol_rule = 1e-13 in its own arithmetic, and its Sigma_z and nu differ from the reference's by the
cancellation in z_i - z_0 (values up to 80 m, deltas down to 0.08: 1024 ulp = 2.3e-13), which cond(S) <= 2000 (asserted by the
CPU test) turns into 2 * 2000 * 2.3e-13 = 9.1e-10 on d^2; wide_arithmetic adds the rounding of the stored lambda, eta 2^-24.
Plain fp32: M_FEAT times what an all-float32 CPU evaluation of the same batch leaves (robust_reference.f32_distances), floor
20 * 2^-24; never a GPU figure.  Every comparison prints a PARITY line before it asserts."""
import numpy as np
import pytest
import torch

import feature_f32 as ff
import feature_scaled_parity as fsp
import robust_reference as rr
import sensor_meas_reference as sr
from engine_support import cycled_engine, dev, man_of, same, same_snapshot, scaled, snapshot, stored, tdt
from sensor_meas_cases import PRECS, case, cycling_ids, engine_of, make_inputs, mixed_z, run, spe_identity

pytestmark = pytest.mark.gpu

ST_NONFINITE, ST_CHOLESKY, ST_UNINIT, ST_INACTIVE, ST_REJECTED = 1 << 4, 1 << 5, 1 << 7, 1 << 8, 1 << 9
FLOAT_KEYS = ("z_pred", "S", "innov", "maha0", "maha", "loglik", "scale")
OUT_KEYS = FLOAT_KEYS + ("iterations", "status")
ALL_KEYS = ("mu", "cov") + OUT_KEYS
SHAPES = {"z_pred": (3,), "S": (9,), "innov": (3,), "maha0": (), "maha": (), "loglik": (), "scale": ()}
MODES = [("match", rr.MATCH), ("huber", rr.HUBER)]


def rules(spe, c, mode=rr.MATCH, chi2_m1=rr.CHI2_M1, chi2_m3=rr.CHI2_M3, scale_max=1e30, max_iter=16):
    """-> (the ctypes rule for the engine, the reference's Rule with the values as the engine's storage holds them)"""
    tol = 2e-6 if c.pname == "f32" else 1e-13
    s = lambda x: float(stored(x, c.dtype))   # noqa: E731
    return (spe.RobustRule(mode, chi2_m1, chi2_m3, scale_max, tol, max_iter),
            rr.rule(mode, s(chi2_m1), s(chi2_m3), s(scale_max), s(tol), max_iter))


def run_robust(e, ids, z, Q, mount, point, rule, commit=True, q_uniform=False, want=OUT_KEYS):
    """-> dict(mu, cov and the outputs in `want`) after update_robust_dev; mount [7] / point [3]: uniform"""
    n, dt = e.capacity, tdt(e)
    zd = dev(e, z)
    qd = dev(e, np.asarray(Q).reshape(9) if q_uniform else np.asarray(Q).reshape(n, 9))
    idd = None if np.isscalar(ids) else torch.from_numpy(np.asarray(ids, dtype=np.int32)).to("cuda")
    mount, point = np.asarray(mount), np.asarray(point)
    md = dev(e, mount) if mount.ndim == 2 else None
    pd = dev(e, point) if point.ndim == 2 else None
    o = {k: torch.full((n,) + SHAPES[k], -7.0, dtype=dt, device="cuda") for k in FLOAT_KEYS if k in want}
    o.update({k: torch.full((n,), -1, dtype=torch.int32, device="cuda") for k in ("iterations", "status") if k in want})
    torch.cuda.synchronize()
    e.update_robust_dev(int(ids) if idd is None else 0, zd, qd, rule, q_is_uniform=q_uniform, model_dev=idd, mount_dev=md,
                        mount=mount if md is None else spe_identity(), point_dev=pd, point=point if pd is None else (0.0, 0.0, 0.0),
                        commit=commit, **o)
    e.sync()
    torch.cuda.synchronize()
    r = {k: v.double().cpu().numpy() for k, v in o.items() if k in FLOAT_KEYS}
    if "S" in r:
        r["S"] = r["S"].reshape(n, 3, 3)
    if "iterations" in o:
        r["iterations"] = o["iterations"].cpu().numpy()
    if "status" in o:
        r["status"] = o["status"].cpu().numpy().astype(np.uint32)
    r["mu"], r["cov"], _ = e.state()
    return r


def contaminated(c, ids):
    """the case's samples with the constructed radii, as the engine stores them; cached on the case"""
    key = ("zc", int(ids) if np.isscalar(ids) else "per-filter")
    if key not in c.refs:
        z0 = c.z[int(ids)] if np.isscalar(ids) else mixed_z(c, ids)
        c.refs[key] = stored(rr.contaminate(man_of(c.model), c.mu, c.cov, ids, z0, c.Q, c.mount, c.point, c.gyro), c.dtype)
    return c.refs[key]


def narrowed(c, ref):
    """the reference's float outputs as a wide_arithmetic engine stores them"""
    if not c.wide:
        return ref
    return {k: (v.astype(np.float32).astype(np.float64) if k in ("mu", "cov") + FLOAT_KEYS else v) for k, v in ref.items()}


def separated(name, d0, c2, gate=None):
    """the decisions of the batch are not rounding's: no raw distance within 10 % of its threshold or of the gate"""
    assert not (np.abs(d0 - c2) <= 0.1 * c2).any(), name
    assert gate is None or not (np.abs(d0 - gate) <= 0.1 * gate).any(), name


def scaled_checks(name, c, ids, z, got, ref, lam_q):
    """the scaled checks of tests/feature_scaled_parity.py on the state and on z-bar, S, nu, against the update that lam_q makes"""
    idv = np.broadcast_to(np.asarray(ids, dtype=np.int64), (c.n,))
    evals = {}

    def f32():
        if not evals:
            for p in ("f32", "f64"):
                evals[p] = ff.sensor_meas(c.model, c.mu, c.cov, idv, z, lam_q, c.mount, c.point, c.gyro, keep=ref["status"] != 0, prec=p)
        return evals
    fsp.judge_state("robust/" + name, c.model, c.pname, got["mu"], got["cov"], ref["mu"], ref["cov"],
                    f32=lambda: tuple((f32()[p]["mu"], f32()[p]["cov"]) for p in ("f32", "f64")))
    scored = ~np.isnan(ref["maha"])
    dims = np.array([sr.meas_dim(int(i)) if i in sr.ids_of(man_of(c.model)) else 0 for i in idv])
    for m in (1, 3):
        sel = scored & (dims == m)
        if sel.any():
            pick = lambda o: (o["z_pred"][sel][:, :m], o["S"][sel][:, :m, :m], o["innov"][sel][:, :m])   # noqa: E731
            fsp.judge_meas(f"robust/{name}/m={m}", c.pname, *pick(got), *pick(ref), f32=lambda: tuple(pick(f32()[p]) for p in ("f32", "f64")))


# ----------------------------------------------------------------------------------------------------------------- inliers
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_inliers_take_the_sensor_update(spe, model, pname):
    """thresholds out of reach: every row is ukfb_update_sensor_dev's on a twin engine"""
    c = case(spe, model, pname)
    ids = cycling_ids(model, c.n)
    z = contaminated(c, ids)
    rule, _ = rules(spe, c, chi2_m1=1e30, chi2_m3=1e30)
    e, twin = engine_of(spe, c), engine_of(spe, c)
    got = run_robust(e, ids, z, c.Q, c.mount, c.point, rule)
    base = run(twin, ids, z, c.Q, c.mount, c.point)
    assert np.array_equal(e.status(), twin.status())
    e.close(); twin.close()
    assert np.array_equal(got["status"], base["status"])
    scored = ~np.isnan(base["maha"])
    assert scored.sum() >= c.n // 2 and np.array_equal(np.isnan(got["maha"]), ~scored)
    err = {k: scaled(got[k], base[k]) for k in ("mu", "cov")}
    err.update({k: scaled(got[k][scored], base[k][scored]) for k in ("z_pred", "S", "innov", "maha", "loglik")})
    bits = same(got, base, ("mu", "cov", "z_pred", "S", "innov", "maha", "loglik"))
    print(f"PARITY robust/{model}/{pname}/inliers-vs-update_sensor n={c.n} " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) +
          f" tol={c.tol:.3e} bit_identical={bits}")
    assert all(v <= c.tol for v in err.values()), err
    assert (got["scale"][scored] == 1.0).all() and np.isnan(got["scale"][~scored]).all()
    assert (got["iterations"] == 0).all()
    assert np.array_equal(got["maha"], got["maha0"], equal_nan=True)
    assert np.isnan(got["maha0"][~scored]).all() and np.isnan(got["loglik"][~scored]).all()


# ------------------------------------------------------------------------------------------------------ contaminated parity
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
@pytest.mark.parametrize("mname,mode", MODES)
def test_contaminated_parity(spe, model, pname, mname, mode):
    """per model id and with an id per filter (wave-mates then differ in model, in m and between 0 and 8 trips; negative ids
    and the other engine's included).  Plain fp32: lambda and the residual against the bounds of the all-float32 evaluation."""
    c = case(spe, model, pname)
    man = man_of(model)
    rule, R = rules(spe, c, mode)
    for ids in list(sr.ids_of(man)) + [cycling_ids(model, c.n)]:
        name = f"{model}/{pname}/{mname}/" + (sr.NAMES[int(ids)] if np.isscalar(ids) else "per-filter-ids")
        idv = np.broadcast_to(np.asarray(ids, dtype=np.int64), (c.n,))
        z = contaminated(c, ids)
        raw = sr.update_sensor(man, c.mu, c.cov, ids, z, c.Q, c.mount, c.point, c.gyro)
        ref = rr.update_robust(man, c.mu, c.cov, ids, z, c.Q, c.mount, c.point, c.gyro, rule=R)
        e = engine_of(spe, c)
        got = run_robust(e, ids, z, c.Q, c.mount, c.point, rule)
        assert np.array_equal(e.status(), got["status"])   # commit = 1 writes the engine's own status array too
        e.close()
        assert np.array_equal(got["status"], ref["status"]), name
        scored = ~np.isnan(ref["maha"])
        c2 = rr.thresholds(idv, R)
        separated(name, ref["maha0"][scored], c2[scored])
        assert np.array_equal(np.isnan(got["maha"]), ~scored) and np.isnan(got["scale"][~scored]).all() and (got["iterations"][~scored] == 0).all()
        infl = scored & (ref["scale"] > 1.0)
        assert infl.sum() >= scored.sum() // 2 and np.array_equal(got["scale"][scored] > 1.0, infl[scored]), name
        assert (got["scale"][scored & ~infl] == 1.0).all() and (got["iterations"][~infl] == 0).all()
        trips = got["iterations"][infl]
        print(f"TRIPS robust/{name} inflated={int(infl.sum())} min={trips.min()} max={trips.max()} mean={trips.mean():.2f}")
        assert trips.max() <= 16 and ((trips >= 1).all() if mode == rr.MATCH else (trips == 0).all())
        # ---- lambda and the scores against the reference
        lam_err = float(np.max(np.abs(got["scale"][infl] - ref["scale"][infl]) / ref["scale"][infl]))
        if pname == "f32":
            d = rr.f32_distances(model, c.mu, c.cov, ids, z, c.Q, c.mount, c.point, c.gyro, R)
            assert np.array_equal(d["rows"], infl), name
            lam_bound = max(fsp.M_FEAT * d["d_lam"], rr.FLOOR_F32)
            print(f"PARITY robust/{name} n={int(infl.sum())} max_rel_dlambda={lam_err:.3e} bound={lam_bound:.3e} (d_32={d['d_lam']:.3e})")
            assert lam_err <= lam_bound, (name, lam_err, lam_bound)
        else:
            r = narrowed(c, ref)
            err = {k: scaled(got[k][scored], r[k][scored]) for k in ("scale", "maha0", "maha", "loglik", "z_pred", "S", "innov")}
            err.update({k: scaled(got[k], r[k]) for k in ("mu", "cov")})
            print(f"PARITY robust/{name} n={int(scored.sum())} max_rel_dlambda={lam_err:.3e} " +
                  " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={c.tol:.3e}")
            assert lam_err <= c.tol and all(v <= c.tol for v in err.values()), (name, lam_err, err)
        # ---- MATCH: the residual of the GPU's lambda, recomputed in float64
        if mode == rr.MATCH:
            Sz, Qe, nu = rr.embed(idv[infl], raw["S"][infl], c.Q[infl], raw["innov"][infl])
            f, _ = rr.evaluate(Sz, Qe, nu, got["scale"][infl])
            resid = float(np.max(np.abs(f - c2[infl]) / c2[infl]))
            bound = max(fsp.M_FEAT * d["d_resid"], rr.FLOOR_F32) if pname == "f32" else c.tol
            print(f"PARITY robust/{name} n={int(infl.sum())} max |d2_fp64(lambda_gpu) - c2| / c2 = {resid:.3e} bound={bound:.3e}")
            assert resid <= bound, (name, resid, bound)
        # ---- every mode: the committed state is update_sensor's with lambda_gpu Q (a solve error cannot hide an update error)
        with_gpu = rr.update_robust(man, c.mu, c.cov, ids, z, c.Q, c.mount, c.point, c.gyro, rule=R, scale=got["scale"])
        assert np.array_equal(with_gpu["status"], got["status"])
        r = narrowed(c, with_gpu)
        err = {k: scaled(got[k], r[k]) for k in ("mu", "cov")}
        err.update({k: scaled(got[k][scored], r[k][scored]) for k in ("z_pred", "S", "innov")})
        print(f"PARITY robust/{name}/update-with-lambda_gpu n={c.n} " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) +
              f" tol={c.tol:.3e}")
        assert all(v <= c.tol for v in err.values()), (name, err)
        # the scaled checks, against the update of the lambda the kernel USED: a plain fp32 engine stores it as it used it; a
        # wide_arithmetic engine used it unrounded, which is the reference's own to the fp64 tolerance above
        judge = with_gpu if pname == "f32" else ref
        lam_q = np.where(scored, judge["scale"], 1.0)[:, None, None] * c.Q
        scaled_checks(name, c, ids, z, got, judge, lam_q)


# --------------------------------------------------------------------------------------------------------------------- cap
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_cap_of_one_step(spe, model):
    """max_iter = 1: m = 1 rows reach d^2 = c^2, m = 3 rows report one step and hold newton_iterates' first iterate"""
    c = case(spe, model, "f64")
    man = man_of(model)
    rule, R = rules(spe, c, max_iter=1)
    for mid in ((sr.POSE_RANGE, sr.POSE_POINT) if model == "pose" else (sr.ORIENT_NAV_VECTOR,)):
        z = contaminated(c, mid)
        raw = sr.update_sensor(man, c.mu, c.cov, mid, z, c.Q, c.mount, c.point, c.gyro)
        e = engine_of(spe, c)
        got = run_robust(e, mid, z, c.Q, c.mount, c.point, rule)
        e.close()
        c2 = R.chi2_m1 if sr.meas_dim(mid) == 1 else R.chi2_m3
        infl = raw["maha"] > c2
        separated(sr.NAMES[mid], raw["maha"], c2)
        assert (got["status"] == 0).all() and infl.sum() > c.n // 2
        assert np.array_equal(got["iterations"], np.where(infl, 1, 0))
        Sz, Qe, nu = rr.embed(np.full(int(infl.sum()), mid), raw["S"][infl], c.Q[infl], raw["innov"][infl])
        it, steps = rr.newton_iterates(Sz, Qe, nu, c2, R.tol, 1)
        assert it.shape[1] == 2 and (steps == 1).all()
        lam_err = float(np.max(np.abs(got["scale"][infl] - it[:, 1]) / it[:, 1]))
        over = (got["maha"][infl] - c2) / c2
        print(f"PARITY robust/{model}/f64/cap/{sr.NAMES[mid]} n={int(infl.sum())} max_rel_dlambda={lam_err:.3e} tol={c.tol:.3e} "
              f"(d2 - c2) / c2: min={over.min():.3e} max={over.max():.3e}")
        assert lam_err <= c.tol
        if sr.meas_dim(mid) == 1:
            assert np.abs(over).max() <= c.tol                       # one step is exact
        else:
            assert (over > -c.tol).all() and (over > R.tol).sum() > infl.sum() // 2   # the iterate has not passed the root; the cap shows


# ---------------------------------------------------------------------------------------------------------- gate and clamp
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", ["f64", "f32"])
def test_gate_and_clamp(spe, model, pname):
    """scale_max is chosen with no root of the batch within 10 % of it.  gate_chi2 = 400 on the raw distance: rho >= 30 is
    REJECTED_GATE with the state kept and scale 1.  Gate off: every clamped row (rho = 300 among them) holds exactly scale_max,
    keeps maha > c^2 and still commits."""
    c = case(spe, model, pname)
    man = man_of(model)
    rho = np.array(rr.RHO)[np.arange(c.n) % len(rr.RHO)]
    for mid in rr.CLAMP_MODELS[model]:
        z = contaminated(c, mid)
        args = (man, c.mu, c.cov, mid, z, c.Q, c.mount, c.point, c.gyro)
        free = rr.update_robust(*args, rule=rules(spe, c)[1])   # the roots themselves
        assert (free["status"] == 0).all()
        scale_max = rr.pick_scale_max(free["scale"][free["scale"] > 1.0])
        rule, R = rules(spe, c, scale_max=scale_max)
        assert R.scale_max == scale_max
        c2 = R.chi2_m1 if sr.meas_dim(mid) == 1 else R.chi2_m3
        separated(sr.NAMES[mid], free["maha0"], c2, rr.GATE)
        for gate in (rr.GATE, -1.0):
            name = f"{model}/{pname}/{sr.NAMES[mid]}/scale_max={scale_max:g}/gate={gate:g}"
            ref = rr.update_robust(*args, rule=R, gate_chi2=gate)
            e = engine_of(spe, c, gate_chi2=gate)
            got = run_robust(e, mid, z, c.Q, c.mount, c.point, rule)
            e.close()
            rej = (rho >= 30.0) & (gate >= 0)
            assert np.array_equal(got["status"], np.where(rej, ST_REJECTED, 0)) and np.array_equal(ref["status"], got["status"])
            assert np.array_equal(got["mu"][rej], c.mu[rej]) and np.array_equal(got["cov"][rej], c.cov[rej])
            assert (got["scale"][rej] == 1.0).all() and (got["iterations"][rej] == 0).all()
            assert np.array_equal(got["maha"][rej], got["maha0"][rej]) and np.isfinite(got["loglik"][rej]).all()
            assert pname != "f64" or scaled(got["maha0"], ref["maha0"]) <= c.tol
            clamped = ~rej & (free["scale"] > scale_max)
            inside = ~rej & (free["scale"] < scale_max) & (free["scale"] > 1.0)
            print(f"PARITY robust/{name} rejected={int(rej.sum())} clamped={int(clamped.sum())} inside={int(inside.sum())}")
            if gate < 0:
                assert rej.sum() == 0 and clamped.sum() >= c.n // 6 and inside.sum() >= c.n // 20   # rho = 300 alone is a sixth
            else:
                assert rej.sum() >= c.n // 4
            assert (got["scale"][clamped] == scale_max).all() and (got["maha"][clamped] > c2).all()
            assert (got["scale"][inside] < scale_max).all() and (got["scale"][inside] > 1.0).all()
            moved = np.any(got["mu"] != c.mu, axis=1)
            assert moved[~rej].all()
            r = rr.update_robust(*args, rule=R, gate_chi2=gate, scale=got["scale"])
            err = {k: scaled(got[k], r[k]) for k in ("mu", "cov") + (("maha", "loglik") if pname == "f64" else ())}
            print(f"PARITY robust/{name}/update-with-lambda_gpu " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) +
                  f" tol={c.tol:.3e}")
            assert all(v <= c.tol for v in err.values()), err


# ---------------------------------------------------------------------------------------------------------------- read-only
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("mname,mode", MODES)
def test_read_only(spe, model, mname, mode):
    """commit = 0 leaves the whole downloadable engine bit for bit; its outputs are the committing twin's"""
    c = case(spe, model, "f64", 255)
    ids = cycling_ids(model, c.n)
    z = contaminated(c, ids)
    rule, _ = rules(spe, c, mode)
    e, twin = engine_of(spe, c), engine_of(spe, c)
    before = snapshot(e)
    dry = run_robust(e, ids, z, c.Q, c.mount, c.point, rule, commit=False)
    assert same_snapshot(before, snapshot(e))
    wet = run_robust(twin, ids, z, c.Q, c.mount, c.point, rule)
    assert same(dry, wet, OUT_KEYS)
    assert np.array_equal(dry["mu"], c.mu) and np.array_equal(dry["cov"], c.cov) and not np.array_equal(wet["mu"], c.mu)
    assert (wet["scale"][~np.isnan(wet["scale"])] > 1.0).sum() > c.n // 4
    # commit = 0, then commit = 1: the same numbers as commit = 1 alone
    assert same(run_robust(e, ids, z, c.Q, c.mount, c.point, rule), wet, ALL_KEYS)
    e.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------- refused filters
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("mname,mode", MODES)
def test_refused_filters_never_move_a_wave_mate(spe, model, mname, mode):
    """One wavefront each: an uninitialised filter, a NaN in z, a NaN in a mount entry the model reads, a Sigma of -I, a Q that
    makes S(1) fail in its leading pivot -- each with three healthy mates at different trip counts"""
    n = 20
    dead, nan_z, nan_m, neg, bad_q = 1, 6, 11, 12, 19
    man = man_of(model)
    mid = sr.POSE_POINT if model == "pose" else sr.ORIENT_VELOCITY   # reads r and qs
    e = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    twin = cycled_engine(spe, model, n, 0, 0)
    mu, cov, init = e.state()
    mu_t, cov_t, _ = twin.state()
    healthy = np.arange(n) != dead
    assert not init[dead] and np.array_equal(mu[healthy], mu_t[healthy]) and np.array_equal(cov[healthy], cov_t[healthy])
    mount, point, gyro, zs, Q = make_inputs(model, mu_t, np.float64)
    if model == "orient":
        e.set_orient_inputs(gyro=gyro); twin.set_orient_inputs(gyro=gyro)
    z = rr.contaminate(man, mu_t, cov_t, mid, zs[mid], Q, mount, point, gyro)
    c = type("C", (), {"pname": "f64", "dtype": np.float64})
    rule, R = rules(spe, c, mode)
    clean = run_robust(twin, mid, z, Q, mount, point, rule)
    twin.close()
    assert (clean["status"] == 0).all() and len(np.unique(clean["iterations"])) >= (2 if mode == rr.MATCH else 1)
    zb, Qb, mb = z.copy(), Q.copy(), mount.copy()
    zb[nan_z, 1] = np.nan
    mb[nan_m, 4] = np.nan
    Qb[bad_q] = -100.0 * np.eye(3)
    cov_bad = cov.copy()
    cov_bad[neg] = -np.eye(man.D)
    e.initialize(mu[neg:neg + 1], cov_bad[neg:neg + 1], first=neg)
    if model == "orient":
        e.set_orient_inputs(gyro=gyro)
    got = run_robust(e, mid, zb, Qb, mb, point, rule)
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[[nan_z, nan_m]], expect[[neg, bad_q]] = ST_UNINIT, ST_NONFINITE, ST_CHOLESKY
    assert np.array_equal(got["status"], expect), (got["status"], expect)
    assert np.array_equal(e.status(), expect)
    e.close()
    ref = rr.update_robust(man, mu_t, cov_bad, mid, zb, Qb, mb, point, gyro, rule=R, initialised=init)
    assert np.array_equal(ref["status"], expect)
    failing = expect != 0
    assert np.array_equal(got["mu"][failing], mu[failing], equal_nan=True)
    keep = failing & (np.arange(n) != neg)
    assert np.array_equal(got["cov"][keep], cov[keep], equal_nan=True) and np.array_equal(got["cov"][neg], cov_bad[neg])
    assert all(np.isnan(got[k][failing]).all() for k in ("z_pred", "S", "maha0", "maha", "loglik", "scale"))
    assert np.isnan(got["innov"][failing]).all() and (got["iterations"][failing] == 0).all()
    assert same(got, clean, ALL_KEYS, rows=~failing)


# --------------------------------------------------------------------------------------------------------- other input forms
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_other_input_forms(spe, model):
    n = 255
    c = case(spe, model, "f64", n)
    man = man_of(model)
    mid = sr.POSE_POINT if model == "pose" else sr.ORIENT_VELOCITY
    mount1, point1 = c.mount[7], c.point[7]
    z = rr.contaminate(man, c.mu, c.cov, mid, c.z[mid], c.Q, mount1, point1, c.gyro)
    rule, R = rules(spe, c)

    def fresh():
        return engine_of(spe, c)

    e = fresh()
    base = run_robust(e, mid, z, c.Q, mount1, point1, rule)
    e.close()
    assert (base["status"] == 0).all() and (base["scale"] > 1.0).sum() > n // 2 and (base["scale"] == 1.0).sum() > n // 4
    # per-filter mount / point arrays that repeat the uniform ones, a device array filled with the id; ONE 3 x 3 for Q
    e = fresh()
    assert same(run_robust(e, np.full(n, mid, dtype=np.int32), z, c.Q, np.tile(mount1, (n, 1)), np.tile(point1, (n, 1)), rule), base, ALL_KEYS)
    e.close()
    e = fresh()
    assert same(run_robust(e, mid, z, c.Q[0], mount1, point1, rule, q_uniform=True), base, ALL_KEYS)
    e.close()
    # any subset of the outputs; none at all with commit = 1
    for want in (("scale",), ("iterations",), ("maha0", "status"), ("S", "innov", "loglik"), ("z_pred", "maha")):
        e = fresh()
        assert same(run_robust(e, mid, z, c.Q, mount1, point1, rule, want=want), base, ("mu", "cov") + want), want
        e.close()
    e = fresh()
    zd, qd = dev(e, z), dev(e, c.Q.reshape(n, 9))
    e.update_robust_dev(mid, zd, qd, rule, mount=mount1, point=point1)
    e.sync()
    m2, C2, _ = e.state()
    assert np.array_equal(m2, base["mu"]) and np.array_equal(C2, base["cov"]) and np.array_equal(e.status(), base["status"])
    with pytest.raises(spe.UkfbError, match="code 1"):   # commit = 0 with nothing to write
        e.update_robust_dev(mid, zd, qd, rule, mount=mount1, point=point1, commit=False)
    with pytest.raises(spe.UkfbError, match="code 1"):   # a rule out of range is refused before any launch
        e.update_robust_dev(mid, zd, qd, spe.RobustRule(0, 3.8, 7.8, 0.5, 1e-13, 16), mount=mount1, point=point1)
    assert np.array_equal(e.state()[0], m2)
    e.close()
    # the host form = the device form (per-filter ids, mounts and points too)
    e = fresh()
    o = e.update_robust(mid, z, c.Q, rule, mount1, point1)
    o["mu"], o["cov"], _ = e.state()
    assert same(o, base, ALL_KEYS)
    e.close()
    per = cycling_ids(model, n)
    zp = contaminated(c, per)
    e, e2 = fresh(), fresh()
    o = e.update_robust(per, zp, c.Q, rule, c.mount, c.point)
    o["mu"], o["cov"], _ = e.state()
    assert same(o, run_robust(e2, per, zp, c.Q, c.mount, c.point, rule), ALL_KEYS)
    e.close(); e2.close()
