"""Sensor-frame measurements on the device (ukfb_update_sensor_dev / ukfb_update_sensor / integrateSensorMeasurement,
include/ukf_batch.h).

States: synth.pose_initial / orient_initial after two real cycles, downloaded and re-uploaded bit for bit.  Inputs (seed 5):
mounts r ~ U(-1, 1)^3, qs = exp(U(-1, 1)^3); points 15 ... 80 m from the filter (OrientationState: from the body origin);
z = h(mu) + 0.05 N(0, 1), Q = 0.05^2 I; OrientationState's latched gyro sample N(0, 0.1^2); everything rounded to the engine's
storage before the reference sees it.  The reference is tests/sensor_meas_reference.py (pinned by
tests/test_sensor_meas_reference.py) run on the state AS DOWNLOADED and the inputs AS STORED.  Parity bound:
|x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64) / 1e-4 (fp32) / 1e-9 + 2^-23 (fp32 engines with wide_arithmetic, against the
reference's outputs rounded to fp32), on mean, covariance, z-bar, S, nu, d^2 and log-likelihood.  Every comparison prints a
PARITY line with its maxima before it asserts.

Every parity comparison also makes the SCALED one (tests/feature_scaled_parity.py): the updated state (mu, C) whitened by the
reference's own sigmas and held block by block -- fp64 1e-9; wide_arithmetic 2 u v + 1e-9 against the float64 reference on the
inputs as stored (the kernel narrows each stored output once); plain fp32 max(M_feat d_32, 20 u v), d_32 the distance of the
all-float32 evaluation of the same call (tests/feature_f32.py) from its float64 evaluation on the same batch.  It prints one
SCALED line: the largest fraction of a bound and the block it belongs to.  z-bar, S and nu are held
the same way at the scale of S (s^z_i = sqrt(S_ref[i, i]); v = 1 for S, |nu_i| / s^z_i, max(1, |z-bar_i|) / s^z_i); d^2 and the
log-likelihood stay on the bound above.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import feature_f32 as ff
import feature_scaled_parity as fsp
import sensor_meas_reference as sr
from engine_support import cycled_engine, man_of, same, same_snapshot, scaled, snapshot, stored
from sensor_meas_cases import (PRECS, Case, case, cycling_ids, engine_of, make_inputs, mixed_z, reference, run, run_case,
                               spe_identity)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_NONFINITE, ST_CHOLESKY, ST_UNINIT, ST_INACTIVE, ST_REJECTED = 1 << 4, 1 << 5, 1 << 7, 1 << 8, 1 << 9
OUT_KEYS = ("z_pred", "S", "innov", "maha", "loglik")
ALL_KEYS = ("mu", "cov") + OUT_KEYS + ("status",)


def check_parity(name, c, got, ref, tol=None, rows=None, ids=None):
    """the file's bound on every output, then the scaled checks of tests/feature_scaled_parity.py: the updated state block by
    block, and z-bar, S, nu at the scale of S; ids: the call's model id(s), for the fp32 evaluation behind a plain fp32
    engine's bound (rows of one measurement dimension are judged together: POSE_RANGE has m = 1)"""
    tol = c.tol if tol is None else tol
    rows = np.ones(c.n, bool) if rows is None else rows
    r = {k: np.asarray(ref[k], dtype=np.float64) for k in ALL_KEYS[:-1]}
    if c.wide:   # the engine stores fp32
        r = {k: v.astype(np.float32).astype(np.float64) for k, v in r.items()}
    scored = rows & ~np.isnan(r["maha"])
    assert np.array_equal(np.isnan(got["maha"][rows]), np.isnan(r["maha"][rows])), name
    err = {k: scaled(got[k][rows], r[k][rows]) for k in ("mu", "cov")}
    err.update({k: scaled(got[k][scored], r[k][scored]) for k in OUT_KEYS})
    print(f"PARITY {name} n={int(rows.sum())} " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={tol:.3e}")
    assert all(v <= tol for v in err.values()), (name, err, tol)
    idv = np.broadcast_to(np.asarray(ids, dtype=np.int64), (c.n,))
    z = c.z[int(ids)] if np.isscalar(ids) else mixed_z(c, ids)
    evals = {}

    def f32():
        if not evals:
            for p in ("f32", "f64"):
                evals[p] = ff.sensor_meas(c.model, c.mu, c.cov, idv, z, c.Q, c.mount, c.point, c.gyro, keep=ref["status"] != 0, prec=p)
        return evals
    fsp.judge_state("sensor_meas/" + name, c.model, c.pname, got["mu"][rows], got["cov"][rows], ref["mu"][rows], ref["cov"][rows],
                    f32=lambda: tuple((f32()[p]["mu"][rows], f32()[p]["cov"][rows]) for p in ("f32", "f64")))
    dims = np.array([sr.meas_dim(int(i)) if i in sr.ids_of(man_of(c.model)) else 0 for i in idv])
    for m in (1, 3):
        sel = scored & (dims == m)
        if sel.any():
            pick = lambda o: (o["z_pred"][sel][:, :m], o["S"][sel][:, :m, :m], o["innov"][sel][:, :m])   # noqa: E731
            fsp.judge_meas(f"sensor_meas/{name}/m={m}", c.pname, *pick(got), *pick(ref), f32=lambda: tuple(pick(f32()[p]) for p in ("f32", "f64")))


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_parity(spe, model, pname):
    c = case(spe, model, pname)
    uniform = {}
    for mid in sr.ids_of(man_of(model)):
        e = engine_of(spe, c)
        got, ref = run_case(e, c, mid), reference(c, mid)
        e.close()
        assert (ref["status"] == 0).all(), (mid, np.unique(ref["status"]))
        assert (got["status"] == 0).all(), (mid, np.unique(got["status"]))
        check_parity(f"{model}/{pname}/{sr.NAMES[mid]}", c, got, ref, ids=mid)
        m = sr.meas_dim(mid)
        assert (got["z_pred"][:, m:] == 0).all() and (got["innov"][:, m:] == 0).all()
        assert (got["S"][:, m:, :] == 0).all() and (got["S"][:, :, m:] == 0).all()
        assert not np.array_equal(got["mu"], c.mu)
        uniform[mid] = got
    # per-filter ids, every wavefront mixed: the bits of the uniform runs filter by filter
    per = cycling_ids(model, c.n)
    e = engine_of(spe, c)
    got = run_case(e, c, per)
    assert np.array_equal(e.status(), got["status"])   # commit = 1 writes the engine's own status array too
    e.close()
    idle = ~np.isin(per, sr.ids_of(man_of(model)))
    assert idle.sum() >= c.n // 7
    assert np.array_equal(got["status"], np.where(idle, ST_INACTIVE, 0))
    assert np.array_equal(got["mu"][idle], c.mu[idle]) and np.array_equal(got["cov"][idle], c.cov[idle])
    assert all(np.isnan(got[k][idle]).all() for k in OUT_KEYS)
    for mid in sr.ids_of(man_of(model)):
        assert same(got, uniform[mid], ALL_KEYS, rows=per == mid), mid
    check_parity(f"{model}/{pname}/per-filter-ids", c, got, reference(c, per), ids=per)


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", ["f64", "f32"])
def test_gate(spe, model, pname):
    """a gate between the batch's smallest and largest d^2: accepted and REJECTED_GATE split as the reference's"""
    c = case(spe, model, pname)
    mid = sr.ids_of(man_of(model))[0]
    free = reference(c, mid)
    gate = float(np.median(free["maha"]))
    assert free["maha"].min() < gate < free["maha"].max()
    ref = reference(c, mid, gate=gate)
    e = engine_of(spe, c, gate_chi2=gate)
    got = run_case(e, c, mid)
    e.close()
    near = np.abs(free["maha"] - gate) <= c.tol * (1.0 + free["maha"])
    assert near.sum() <= c.n // 100, int(near.sum())
    rows = ~near
    assert np.array_equal(got["status"][rows], ref["status"][rows])
    rej = rows & (ref["status"] == ST_REJECTED)
    assert rej.sum() > c.n // 4 and (rows & (ref["status"] == 0)).sum() > c.n // 4
    assert np.array_equal(got["mu"][rej], c.mu[rej]) and np.array_equal(got["cov"][rej], c.cov[rej])
    assert np.isfinite(got["maha"][rej]).all()
    check_parity(f"{model}/{pname}/gate", c, got, ref, rows=rows, ids=mid)


# ------------------------------------------------------------------------------------------------------- bit-level properties
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_bit_level_properties(spe, model, tmp_path):
    n = 255
    c = case(spe, model, "f64", n)
    per = cycling_ids(model, n)
    mid = sr.ids_of(man_of(model))[0] + 2 if model == "pose" else sr.ORIENT_VELOCITY   # POSE_POINT / ORIENT_VELOCITY: read mount (and point)
    mount1, point1 = c.mount[7], c.point[7]

    def fresh(**kw):
        e = engine_of(spe, c, **kw)
        e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
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
    e = fresh()
    assert same(run(e, mid, c.z[mid], c.Q[0], mount1, point1, q_uniform=True), base, ALL_KEYS)
    e.close()
    # a gate nothing reaches = no gate
    e = fresh(gate_chi2=1e300)
    assert same(run(e, mid, c.z[mid], c.Q, mount1, point1), base, ALL_KEYS)
    e.close()
    # the host form = the device form (per-filter ids, mounts and points too)
    e = fresh()
    o = e.update_sensor(mid, c.z[mid], c.Q, mount1, point1)
    o["mu"], o["cov"], _ = e.state()
    assert same(o, base, ALL_KEYS)
    e.close()
    e, e2 = fresh(), fresh()
    o = e.update_sensor(per, mixed_z(c, per), c.Q, c.mount, c.point)
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
    assert np.array_equal(dry_per["status"], np.where(np.isin(per, sr.ids_of(man_of(model))), 0, ST_INACTIVE))
    e.predict(0.013); twin.predict(0.013)
    assert same_snapshot(snapshot(e), snapshot(twin))
    e.close(); twin.close()
    # commit = 0, then commit = 1: the same numbers as commit = 1 alone
    e = fresh()
    run(e, mid, c.z[mid], c.Q, mount1, point1, commit=False)
    assert same(run(e, mid, c.z[mid], c.Q, mount1, point1), base, ALL_KEYS)
    e.close()
    # integrateSensorMeasurement of include/pose_estimation/Batch.hpp from a C++ host: the same bits
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the C++ host"
    exe = tmp_path / "sensor_meas_classes"
    lib_dir = os.path.join(ROOT, "slam-pose_estimation_amd", "lib")
    subprocess.run([gxx, "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "sensor_meas_classes.cpp"), "-o", str(exe), "-L", lib_dir, "-lukf_batch",
                    "-Wl,-rpath," + lib_dir], check=True, timeout=300)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    gyro = c.gyro if model == "orient" else np.zeros((n, 3))
    with open(fin, "wb") as f:
        np.array([n, 0 if model == "pose" else 1, mid], dtype=np.int64).tofile(f)
        for a in (c.mu, c.cov, gyro, c.z[mid], c.Q, mount1, point1):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    out = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(fout, dtype=np.float64)
    S, D = man_of(model).S, man_of(model).D
    sizes = [("mu", (n, S)), ("cov", (n, D, D)), ("z_pred", (n, 3)), ("S", (n, 3, 3)), ("innov", (n, 3)), ("maha", (n,)),
             ("loglik", (n,)), ("status", (n,))]
    o, at = {}, 0
    for k, shape in sizes:
        cnt = int(np.prod(shape))
        o[k] = raw[at:at + cnt].reshape(shape)
        at += cnt
    assert at == raw.size
    o["status"] = o["status"].astype(np.uint32)
    assert same(o, base, ALL_KEYS)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_small_batches(spe, model):
    """1, 2, 3 and 5 filters: one partly filled wavefront, and a full one with a one-row tail"""
    big = case(spe, model, "f64", 255)
    for n in (1, 2, 3, 5):
        for mid in sr.ids_of(man_of(model)):
            c = Case()
            c.model, c.pname, c.n, c.prec, c.wide, c.tol, c.dtype = model, "f64", n, 0, 0, 1e-9, big.dtype
            c.mu, c.cov, c.mount, c.point, c.gyro, c.Q = big.mu[:n], big.cov[:n], big.mount[:n], big.point[:n], big.gyro[:n], big.Q[:n]
            c.z = {mid: big.z[mid][:n]}
            e = engine_of(spe, c)
            got = run_case(e, c, mid)
            e.close()
            ref = sr.update_sensor(man_of(model), c.mu, c.cov, mid, c.z[mid], c.Q, c.mount, c.point, c.gyro)
            assert (got["status"] == 0).all() and (ref["status"] == 0).all()
            check_parity(f"{model}/f64/{sr.NAMES[mid]}/n={n}", c, got, ref, ids=mid)


@pytest.mark.parametrize("pname", ["f32", "f32w"])
def test_host_array_form_fp32(spe, pname):
    """fp32 engines: ukfb_update_sensor narrows the host doubles itself; its outputs and the committed state are the bits of
    the device form fed the same values rounded to float32.  Five filters."""
    n = 5
    c = case(spe, "pose", pname, n)
    rng = np.random.default_rng(9)
    mid = sr.POSE_POINT
    z = c.z[mid] + 1e-3 * rng.standard_normal((n, 3))          # doubles that are NOT fp32 values
    mount = c.mount + 1e-3 * rng.standard_normal((n, 7))
    point = c.point + 1e-3 * rng.standard_normal((n, 3))
    assert not np.array_equal(z, stored(z, np.float32))
    for mt, pt in ((mount, point), (mount[2], point[2])):
        e, twin = engine_of(spe, c), engine_of(spe, c)
        o = e.update_sensor(mid, z, c.Q, mt, pt)
        o["mu"], o["cov"], _ = e.state()
        dev = run(twin, mid, stored(z, np.float32), c.Q, stored(mt, np.float32), stored(pt, np.float32))
        assert same(o, dev, ALL_KEYS) and np.array_equal(e.status(), twin.status()) and (o["status"] == 0).all()
        e.close(); twin.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failures_stay_inside_their_filter(spe, model):
    """Ordinary status paths: NaN in a used entry of z, Q, mount or point, an uninitialised filter, a covariance with a negative
    pivot, an inactive id; NaN in unused entries changes nothing; the wave-mates of each keep the bits of a clean run"""
    n, dead = 64, 22
    nan_z, nan_q, nan_m, nan_p, neg, idle, unused = 13, 17, 25, 30, 34, 38, (41, 42, 43)   # every one in another wavefront's row
    man = man_of(model)
    e = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    mu, cov, init = e.state()
    assert not init[dead] and init.sum() == n - 1
    mu_f = mu.copy()
    mu_f[dead] = mu[0]   # (the dead filter's inputs are made from a neighbour's state: they are never used)
    mount, point, gyro, zs, Q = make_inputs(model, mu_f, np.float64)
    if model == "orient":
        e.set_orient_inputs(gyro=gyro)
    # ids that read everything there is to poison: POSE_POINT (r, qs, b) / ORIENT_VELOCITY (r, qs) and ORIENT_NAV_VECTOR (qs, b)
    ids = np.full(n, sr.POSE_POINT if model == "pose" else sr.ORIENT_VELOCITY, dtype=np.int32)
    if model == "orient":
        ids[nan_p] = sr.ORIENT_NAV_VECTOR
    rng_id = sr.POSE_RANGE if model == "pose" else sr.ORIENT_SPECIFIC_FORCE
    ids[list(unused)] = [rng_id, sr.POSE_VELOCITY if model == "pose" else sr.ORIENT_VELOCITY, sr.POSE_NAV_VELOCITY if model == "pose" else sr.ORIENT_SPECIFIC_FORCE]
    z = np.zeros((n, 3))
    for mid in sr.ids_of(man_of(model)):
        z[ids == mid] = zs[mid][ids == mid]
    snap = e.state()
    clean = run(e, ids, z, Q, mount, point, commit=False)
    assert np.array_equal(clean["status"], np.where(np.arange(n) == dead, ST_UNINIT, 0))
    zb, Qb, mb, pb, ib = z.copy(), Q.copy(), mount.copy(), point.copy(), ids.copy()
    zb[nan_z, 1] = np.nan
    Qb[nan_q, 2, 0] = np.nan
    mb[nan_m, 4] = np.nan
    pb[nan_p, 2] = np.nan
    ib[idle] = -1
    # unused entries: z[1..2] and Q outside [0][0] of RANGE (Pose) / the mount and point of SPECIFIC_FORCE (OrientationState);
    # the point of the VELOCITY models; mount and point of NAV_VELOCITY / SPECIFIC_FORCE
    if model == "pose":
        zb[unused[0], 1:] = np.nan
        Qb[unused[0], 1:, :] = Qb[unused[0], :, 1:] = np.nan
        mb[unused[0], 3:7] = np.nan
    else:
        mb[unused[0], :], pb[unused[0], :] = np.nan, np.nan
    pb[unused[1], :] = np.nan
    mb[unused[2], :], pb[unused[2], :] = np.nan, np.nan
    # a covariance with a negative pivot goes in through initialize
    cov_bad = cov.copy()
    cov_bad[neg] = -np.eye(man.D)
    e.initialize(snap[0][neg:neg + 1], cov_bad[neg:neg + 1], first=neg)
    if model == "orient":
        e.set_orient_inputs(gyro=gyro)
    got = run(e, ib, zb, Qb, mb, pb)
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[neg], expect[idle] = ST_UNINIT, ST_CHOLESKY, ST_INACTIVE
    expect[[nan_z, nan_q, nan_m, nan_p]] = ST_NONFINITE
    assert np.array_equal(got["status"], expect), (got["status"], expect)
    assert np.array_equal(e.status(), expect)
    failing = expect != 0
    assert np.array_equal(got["mu"][failing], snap[0][failing], equal_nan=True)
    keep = failing & (np.arange(n) != neg)
    assert np.array_equal(got["cov"][keep], cov[keep], equal_nan=True) and np.array_equal(got["cov"][neg], cov_bad[neg])
    assert all(np.isnan(got[k][failing]).all() for k in ("z_pred", "S", "maha", "loglik")) and np.isnan(got["innov"][failing, 0]).all()
    # everyone else, the filters with NaN in unused entries included: the bits of a clean committing run on a twin
    twin = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    if model == "orient":
        twin.set_orient_inputs(gyro=gyro)
    ok = run(twin, ids, z, Q, mount, point)
    twin.close(); e.close()
    assert same(ok, clean, OUT_KEYS + ("status",))
    assert same(got, ok, ALL_KEYS, rows=~failing)
    for i in unused:
        assert not np.array_equal(got["mu"][i], mu[i])
    ref = sr.update_sensor(man, mu_f, cov_bad, ib, zb, Qb, mb, pb, gyro, initialised=init)
    assert np.array_equal(ref["status"], expect)


# ------------------------------------------------------------------------------------- consistency with the existing kernels
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_degenerate_mount_agrees_with_update_dev(spe, pname):
    """r = 0, qs the identity: POSE_POSITION / POSE_VELOCITY / ORIENT_VELOCITY against ukfb_update_dev with POS3 / VEL3 /
    ORIENT_BODYVEL3 on a twin engine, within 2 tol"""
    ident = np.array(spe_identity())
    for model, sid, mid in (("pose", sr.POSE_POSITION, spe.MEAS_POS3), ("pose", sr.POSE_VELOCITY, spe.MEAS_VEL3),
                            ("orient", sr.ORIENT_VELOCITY, spe.MEAS_ORIENT_BODYVEL3)):
        c = case(spe, model, pname)
        rng = np.random.default_rng(23)
        z = stored(sr.h(sid, c.mu, ident, np.zeros(3), c.gyro) + 0.05 * rng.standard_normal((c.n, 3)), c.dtype)
        e, twin = engine_of(spe, c), engine_of(spe, c)
        got = run(e, sid, z, c.Q, ident, np.zeros(3))
        twin.update(mid, z, c.Q)
        mu_t, cov_t, _ = twin.state()
        assert (got["status"] == 0).all() and twin.status_summary() == 0
        e.close(); twin.close()
        em, ec = scaled(got["mu"], mu_t), scaled(got["cov"], cov_t)
        print(f"PARITY {model}/{pname}/{sr.NAMES[sid]}-vs-update_dev n={c.n} max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e} tol={2 * c.tol:.3e}")
        assert em <= 2 * c.tol and ec <= 2 * c.tol, (sid, em, ec)
        # and the sensor-frame kernel's result against the reference of ITS call
        d = Case()
        d.__dict__.update(c.__dict__)
        d.z, d.mount, d.point = {sid: z}, np.tile(ident, (c.n, 1)), np.zeros((c.n, 3))
        ref = sr.update_sensor(man_of(model), c.mu, c.cov, sid, z, c.Q, d.mount, d.point, c.gyro)
        assert (ref["status"] == 0).all()
        check_parity(f"{model}/{pname}/{sr.NAMES[sid]}-degenerate-mount", d, got, ref, ids=sid)


def test_uniform_id_of_the_other_engine_is_refused(spe):
    for model, wrong in (("pose", sr.ORIENT_VELOCITY), ("orient", sr.POSE_POSITION), ("pose", -1), ("orient", 8)):
        c = case(spe, model, "f64", 255)
        e = engine_of(spe, c)
        with pytest.raises(spe.UkfbError, match="code 5"):
            run(e, wrong, c.z[sr.ids_of(man_of(model))[0]], c.Q, c.mount, c.point)
        assert np.array_equal(e.state()[0], c.mu)
        e.close()
