"""Covariance conditioning on the device (ukfb_condition_dev and its host form, include/ukf_batch.h).

States: those of tests/sensor_meas_cases.py (synth.pose_initial / orient_initial after two real cycles, downloaded; its `case`
cache is shared).  Every filter's covariance is replaced on the host through its correlation eigen-decomposition
(tests/condition_reference.make_batch, rounded to the engine's storage) and uploaded with initialize, which stores any matrix.
Four quarters: (a) untouched, (b) lambda_min = -1e-3, (c) two eigenvalues at -0.3 and -0.05, (d) lambda_min = eps / 8 with one
diagonal entry below the floor.  eps = 1e-10 (fp64 storage) / 1e-4 (fp32 storage).  The reference is
tests/condition_reference.py (pinned by tests/test_condition_reference.py), its eigh form, run on the state AS DOWNLOADED; it must
find every filter's verdict unambiguous (eig_min <= eps / 4 or eig_min >= eps).  Parity bound: |x - ref| <= tol (1 + |ref|), tol =
1e-9 (fp64) / 1e-4 (fp32) / 1e-9 + 2^-23 (wide_arithmetic, against the reference's outputs rounded to fp32), on eig_min, eig_max
and on the covariance entries divided by s_i s_j (the sigmas of the call: correlation scale).  Every comparison prints a PARITY
line with its maxima before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import condition_reference as cr
import sensor_meas_cases as smc
from engine_support import ACC_COV, dev, host, man_of, new_engine, same, same_snapshot, scaled, snapshot, stored, tdt, unpack
from probe_support import LDS_PATTERNS, lds_poison

pytestmark = pytest.mark.gpu

N = smc.N   # 1022: not a multiple of four
PRECS = smc.PRECS
EPS = {"f64": 1e-10, "f32": 1e-4, "f32w": 1e-4}
ST_NONFINITE, ST_CHOLESKY, ST_UNINIT, ST_INACTIVE, ST_REPAIRED = 1 << 4, 1 << 5, 1 << 7, 1 << 8, 1 << 11
OUT_KEYS = ("eig_min", "eig_max", "out_mu", "out_cov", "status")
ALL_KEYS = ("mu", "cov") + OUT_KEYS


class Batch:
    """a case of sensor_meas_cases with its covariances replaced: mu, cov as the engine stores them, the floor, the quarters"""


_BATCHES = {}


def batch(spe, model, pname, n=N):
    key = (model, pname, n)
    if key not in _BATCHES:
        c = smc.case(spe, model, pname, n)
        b = Batch()
        b.c, b.model, b.pname, b.n, b.tol, b.wide, b.dtype, b.eps = c, model, pname, n, c.tol, c.wide, c.dtype, EPS[pname]
        b.man = man_of(model)
        b.mu = c.mu
        b.cov, b.v, b.quarter = cr.make_batch(c.cov, b.eps, c.dtype)
        b.u_storage = cr.U64 if c.dtype == np.float64 else cr.U32
        _BATCHES[key] = b
    return _BATCHES[key]


def engine_of(spe, b, mu=None, cov=None, skip=(), **kw):
    """a fresh engine holding (mu, cov) of the batch bit for bit; filters in `skip` stay uninitialised"""
    c = b.c
    mu, cov = b.mu if mu is None else mu, b.cov if cov is None else cov
    e = new_engine(spe, c.model, mu.shape[0], c.prec, c.wide, **kw)
    if skip:
        for i in range(mu.shape[0]):
            if i not in skip:
                e.initialize(mu[i:i + 1], cov[i:i + 1], first=i)
    else:
        e.initialize(mu, cov)
    if c.model == "orient":
        e.set_orient_inputs(gyro=c.gyro[:mu.shape[0]])
    m, P, init = e.state()
    keep = init.astype(bool)
    assert np.array_equal(m[keep], mu[keep], equal_nan=True) and np.array_equal(P[keep], cov[keep], equal_nan=True)   # as downloaded
    return e


def run(e, v, eps, select=None, renorm=False, commit=True, outs=True):
    """-> dict(mu, cov: the engine's state after the call; eig_min, eig_max, out_mu, out_cov, status: the call's outputs)"""
    n, dt, D = e.capacity, tdt(e), e.D
    vd = dev(e, v)
    sd = None if select is None else torch.from_numpy(np.asarray(select, dtype=np.uint8)).to("cuda")
    o = {}
    if outs:
        o = {"eig_min": torch.full((n,), -7.0, dtype=dt, device="cuda"), "eig_max": torch.full((n,), -7.0, dtype=dt, device="cuda"),
             "mu": torch.full((n, e.S), -7.0, dtype=dt, device="cuda"),
             "cov_packed": torch.full((n, D * (D + 1) // 2), -7.0, dtype=dt, device="cuda"),
             "status": torch.full((n,), -1, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    e.condition_dev(vd, eps, select_dev=sd, renormalize_quaternion=renorm, commit=commit, **o)
    e.sync()
    torch.cuda.synchronize()
    r = {}
    if outs:
        r = {"eig_min": host(o["eig_min"]), "eig_max": host(o["eig_max"]), "out_mu": host(o["mu"]),
             "out_cov": unpack(host(o["cov_packed"]), D), "status": o["status"].cpu().numpy().astype(np.uint32)}
    r["mu"], r["cov"], _ = e.state()
    return r


def reference(b, mu=None, cov=None, **kw):
    return cr.condition(b.man, b.mu if mu is None else mu, b.cov if cov is None else cov, b.v, b.eps, u_storage=b.u_storage, **kw)


def check_parity(name, b, got, ref, cov_in=None, rows=None):
    """the file's bound on eig_min, eig_max, the covariance output and the engine's covariance, correlation-scaled"""
    cov_in = b.cov if cov_in is None else cov_in
    rows = np.ones(cov_in.shape[0], bool) if rows is None else rows
    _, s, _, _ = cr.correlation(cov_in, b.v)
    scale = (s[:, :, None] * s[:, None, :])[rows]
    r = {k: np.asarray(ref[k], dtype=np.float64)[rows] for k in ("eig_min", "eig_max", "cov")}
    if b.wide:   # the engine stores fp32
        r = {k: v.astype(np.float32).astype(np.float64) for k, v in r.items()}
    err = {"eig_min": scaled(got["eig_min"][rows], r["eig_min"]), "eig_max": scaled(got["eig_max"][rows], r["eig_max"]),
           "out_cov": scaled(got["out_cov"][rows] / scale, r["cov"] / scale), "cov": scaled(got["cov"][rows] / scale, r["cov"] / scale)}
    print(f"PARITY condition {name} n={int(rows.sum())} " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={b.tol:.3e}")
    assert all(v <= b.tol for v in err.values()), (name, err, b.tol)


_RUNS = {}


def committed(spe, b):
    """the committing run on a fresh engine of the batch, made once"""
    key = (b.model, b.pname, b.n)
    if key not in _RUNS:
        e = engine_of(spe, b)
        _RUNS[key] = run(e, b.v, b.eps)
        assert np.array_equal(e.status(), _RUNS[key]["status"])   # commit = 1 writes the engine's own status array too
        e.close()
    return _RUNS[key]


def inputs_of(spe, e, model, mu, cycle=2):
    """the per-cycle inputs a predict needs"""
    sy, n = spe.synth, mu.shape[0]
    if model == "pose":
        e.set_acceleration(sy.pose_cycle_inputs(n, cycle, mu[:, :3])[0], ACC_COV)
    else:
        gyro, acc, _, _ = sy.orient_cycle_inputs(n, cycle, mu[:, 0:4])
        e.set_orient_inputs(gyro, acc)


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_parity(spe, model, pname):
    b = batch(spe, model, pname)
    ref = reference(b)
    # the verdict is unambiguous for every filter, and the quarters are what they claim
    assert ((ref["eig_min"] <= b.eps / 4) | (ref["eig_min"] >= b.eps)).all()
    assert np.array_equal(ref["status"], np.where(b.quarter == 0, 0, ST_REPAIRED))
    got = committed(spe, b)
    assert np.array_equal(got["status"], ref["status"]), np.nonzero(got["status"] != ref["status"])[0][:10]
    check_parity(f"{model}/{pname}", b, got, ref)
    for q in range(4):
        check_parity(f"{model}/{pname}/quarter={'abcd'[q]}", b, got, ref, rows=b.quarter == q)
    # the call's own outputs are the committed numbers; a healthy filter keeps every bit, the mean is never touched
    assert np.array_equal(got["out_cov"], got["cov"]) and np.array_equal(got["out_mu"], got["mu"])
    healthy = b.quarter == 0
    assert np.array_equal(got["cov"][healthy], b.cov[healthy]) and np.array_equal(got["mu"], b.mu)
    assert not np.array_equal(got["cov"][~healthy], b.cov[~healthy])
    assert np.array_equal(got["cov"], np.swapaxes(got["cov"], 1, 2))
    # the repaired diagonal is never below the floor
    assert (np.einsum("bii->bi", got["cov"]) >= b.v).all()
    # the literal Jacobi of the reference: the same verdicts, C' within the bound of the eigh form
    jac = reference(b, method="jacobi")
    assert np.array_equal(jac["status"], ref["status"]) and jac["sweeps"].max() <= cr.MAX_SWEEPS
    check_parity(f"{model}/{pname}/jacobi-reference", b, got, jac)


# ---------------------------------------------------------------------------------------------------------------- 2. recovery
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_recovery(spe, model, pname):
    """The test that needs the feature: ukfb_predict fails on the filters of quarter (b) and would fail for good; after
    condition_dev(commit = 1) the same predict succeeds for every filter."""
    b = batch(spe, model, pname)
    e = engine_of(spe, b)
    inputs_of(spe, e, model, b.mu)
    e.predict(0.01)
    st = e.status()
    assert ((st[b.quarter == 1] & ST_CHOLESKY) != 0).all() and ((st[b.quarter == 2] & ST_CHOLESKY) != 0).all()
    assert (st[b.quarter == 0] == 0).all()
    lost = (st & ST_CHOLESKY) != 0
    mu1, cov1, _ = e.state()
    assert np.array_equal(cov1[lost], b.cov[lost]) and np.array_equal(mu1[lost], b.mu[lost])   # a failing filter keeps its state
    e.predict(0.01)
    assert ((e.status() & ST_CHOLESKY) != 0)[lost].all()   # ... and fails again
    got = run(e, b.v, b.eps)
    assert (got["status"][lost] == ST_REPAIRED).all() and np.isin(got["status"], (0, ST_REPAIRED)).all()
    e.predict(0.01)
    st = e.status()
    print(f"PARITY condition recovery {model}/{pname} n={b.n} lost={int(lost.sum())} after: nonzero={int((st != 0).sum())}")
    assert (st == 0).all(), np.unique(st)
    mu2, cov2, _ = e.state()
    assert np.isfinite(cov2).all() and not np.array_equal(cov2[lost], got["cov"][lost])
    e.close()


# ------------------------------------------------------------------------------------------------------------- 3. idempotence
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_second_call_finds_every_filter_healthy(spe, model, pname):
    b = batch(spe, model, pname)
    first = committed(spe, b)
    e = engine_of(spe, b, mu=first["mu"], cov=first["cov"])
    again = run(e, b.v, b.eps)
    e.close()
    print(f"PARITY condition second call {model}/{pname} n={b.n} eig_min / eps: min={np.min(again['eig_min']) / b.eps:.4f}")
    assert (again["status"] == 0).all(), np.unique(again["status"], return_counts=True)
    assert np.array_equal(again["cov"], first["cov"]) and np.array_equal(again["mu"], first["mu"])
    assert np.array_equal(again["out_cov"], first["cov"]) and np.array_equal(again["out_mu"], first["mu"])
    assert (again["eig_min"] >= 0.5 * b.eps).all()


# ---------------------------------------------------------------------------------------------------------------- 4. commit = 0
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_read_only_mode(spe, model):
    """commit = 0 leaves everything of the engine that can be downloaded bit-identical and returns the outputs of commit = 1 bit for
    bit; commit = 1 without `out` commits the same numbers; times and noise tables are never touched"""
    b = batch(spe, model, "f64", 255)
    base = committed(spe, b)
    stamps = np.arange(1, b.n + 1, dtype=np.int64) * 1000 + 7
    e = engine_of(spe, b)
    e.set_last_measurement_time(stamps)
    before = snapshot(e)
    dry = run(e, b.v, b.eps, commit=False)
    assert same_snapshot(before, snapshot(e))
    assert same(dry, base, OUT_KEYS) and np.array_equal(dry["mu"], b.mu) and np.array_equal(dry["cov"], b.cov)
    alone = run(e, b.v, b.eps, outs=False)
    assert same(alone, base, ("mu", "cov")) and np.array_equal(e.status(), base["status"])
    after = snapshot(e)
    assert np.array_equal(e.last_measurement_time(), stamps)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before[4:], after[4:]))
    e.close()
    # select = NULL equals all ones
    e = engine_of(spe, b)
    assert same(run(e, b.v, b.eps, select=np.ones(b.n, dtype=np.uint8)), base, ALL_KEYS)
    e.close()


# ---------------------------------------------------------------------------------- 5. failures stay inside their filter
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failures_stay_inside_their_filter(spe, model):
    """select = 0, an uninitialised filter, a NaN in the lower triangle: each in a wavefront of its own with three wave-mates,
    which give the bits of a run in which that filter is healthy; a NaN in the upper triangle changes nothing.  fp64 and fp32."""
    for pname in ("f64", "f32"):
        b = batch(spe, model, pname, 64)
        n, D = b.n, b.man.D
        idle, dead, nanf, upper = 13, 22, 34, 41   # every one in another wavefront
        twin = engine_of(spe, b)
        clean = run(twin, b.v, b.eps)
        twin.close()
        cov = b.cov.copy()
        cov[nanf, D - 1, 0] = cov[nanf, 0, D - 1] = np.nan
        e = engine_of(spe, b, cov=cov, skip=(dead,))
        # (initialize mirrors nothing: the upper triangle is not stored, so `upper` is poisoned on the reference's side only)
        sel = np.ones(n, dtype=np.uint8)
        sel[idle] = 0
        mu_b, cov_b, init = e.state()
        assert not init[dead] and init.sum() == n - 1
        got = run(e, b.v, b.eps, select=sel)
        expect = clean["status"].copy()
        expect[idle], expect[dead], expect[nanf] = ST_INACTIVE, ST_UNINIT, ST_CHOLESKY
        assert np.array_equal(got["status"], expect), (got["status"], expect)
        assert np.array_equal(e.status(), expect)
        e.close()
        failing = np.zeros(n, bool)
        failing[[idle, dead, nanf]] = True
        assert np.array_equal(got["mu"][failing], mu_b[failing], equal_nan=True)
        assert np.array_equal(got["cov"][failing], cov_b[failing], equal_nan=True)
        for k in ("eig_min", "eig_max", "out_mu", "out_cov"):
            assert np.isnan(got[k][failing]).all(), k
        assert same(got, clean, ALL_KEYS, rows=~failing)
        cov_r = cov.copy()
        cov_r[upper, 0, D - 1] = np.inf   # never read
        ref = cr.condition(b.man, b.mu, cov_r, b.v, b.eps, select=sel, initialised=init)
        assert np.array_equal(ref["status"], expect)


# --------------------------------------------------------------------------------------------------------------- 6. bad floor
def test_bad_floor(spe):
    for pname in ("f64", "f32w"):
        b = batch(spe, "pose", pname, 64)
        sel = np.ones(b.n, dtype=np.uint8)
        sel[5] = 0
        for bad in (0.0, -1e-6, np.nan, np.inf):
            v = b.v.copy()
            v[b.man.D - 1] = bad
            e = engine_of(spe, b)
            got = run(e, v, b.eps, select=sel)
            assert np.array_equal(got["status"], np.where(sel != 0, ST_NONFINITE, ST_INACTIVE)), bad
            assert np.array_equal(e.status(), got["status"])
            e.close()
            assert np.array_equal(got["mu"], b.mu) and np.array_equal(got["cov"], b.cov)
            for k in ("eig_min", "eig_max", "out_mu", "out_cov"):
                assert np.isnan(got[k]).all(), (bad, k)


# ----------------------------------------------------------------------------------------------------------- 7. small batches
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_small_batches(spe, model):
    """1, 3 and 5 filters: a partly filled wavefront, and a full one with a one-row tail; the same bits as in the batch of 255"""
    big = batch(spe, model, "f64", 255)
    full = committed(spe, big)
    ref = reference(big)
    first = [int(np.nonzero(big.quarter == q)[0][0]) for q in (1, 0, 2, 3)] + [int(np.nonzero(big.quarter == 1)[0][1])]
    for n in (1, 3, 5):
        pick = np.array(first[:n])
        e = engine_of(spe, big, mu=big.mu[pick], cov=big.cov[pick])
        got = run(e, big.v, big.eps)
        e.close()
        sub = {k: ref[k][pick] for k in ("eig_min", "eig_max", "cov", "status")}
        assert np.array_equal(got["status"], sub["status"])
        check_parity(f"{model}/f64/n={n}", big, got, sub, cov_in=big.cov[pick])
        assert all(np.array_equal(got[k], full[k][pick]) for k in ALL_KEYS), n


# ----------------------------------------------------------------------------------------------------------- 8. renormalisation
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_quaternion_renormalisation(spe, model, pname):
    """odd filters: the quaternion scaled by 1 + 1e-3 comes back with | |q|^2 - 1 | inside the rule of the header (8 u of the
    storage type), the same direction, REPAIRED; even filters: a unit quaternion rounded to storage keeps its bits, status 0.
    Nothing else of the mean moves, the healthy covariance keeps its bits; with the flag off nothing of the mean moves."""
    b = batch(spe, model, pname, 64)
    Q, n, u = cr.quat_offset(b.man), b.n, b.u_storage
    unit = b.mu[:, Q:Q + 4] / np.linalg.norm(b.mu[:, Q:Q + 4], axis=1, keepdims=True)
    mu = b.mu.copy()
    mu[:, Q:Q + 4] = unit
    odd = np.arange(n) % 2 == 1
    mu[odd, Q:Q + 4] *= 1.0 + 1e-3
    mu = stored(mu, b.dtype)
    healthy = b.c.cov   # every filter of quarter (a)'s kind
    e = engine_of(spe, b, mu=mu, cov=healthy)
    got = run(e, b.v, b.eps, renorm=True)
    ref = cr.condition(b.man, mu, healthy, b.v, b.eps, renormalize=True, u_storage=u)
    assert np.array_equal(ref["status"], np.where(odd, ST_REPAIRED, 0))
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(e.status(), ref["status"])
    assert np.array_equal(got["mu"][~odd], mu[~odd]) and np.array_equal(got["cov"], healthy) and np.array_equal(got["out_cov"], healthy)
    assert np.array_equal(got["out_mu"], got["mu"])
    others = np.ones(b.man.S, bool)
    others[Q:Q + 4] = False
    assert np.array_equal(got["mu"][:, others], mu[:, others])
    qn = got["mu"][odd, Q:Q + 4]
    norm_err, dir_err = np.abs(np.sum(qn * qn, axis=1) - 1.0).max(), np.abs(qn - unit[odd]).max()
    ref_err = scaled(got["mu"], stored(ref["mu"], b.dtype) if b.wide else ref["mu"])
    print(f"PARITY condition renormalise {model}/{pname} n={n} | |q|^2 - 1 |={norm_err:.3e} direction={dir_err:.3e} rule={8 * u:.3e} "
          f"max_scaled_dmu={ref_err:.3e} tol={b.tol:.3e}")
    assert norm_err <= 8 * u and dir_err <= 4 * u and ref_err <= b.tol
    # the second call leaves every bit; the flag off never looks at the mean
    again = run(e, b.v, b.eps, renorm=True)
    assert (again["status"] == 0).all() and np.array_equal(again["mu"], got["mu"])
    e.close()
    e = engine_of(spe, b, mu=mu, cov=healthy)
    off = run(e, b.v, b.eps)
    e.close()
    assert (off["status"] == 0).all() and np.array_equal(off["mu"], mu) and np.array_equal(off["out_mu"], mu)
    # a zero and a non-finite quaternion: like a non-finite covariance
    bad = mu.copy()
    bad[3, Q:Q + 4] = 0.0
    bad[8, Q + 2] = np.inf
    e = engine_of(spe, b, mu=bad, cov=healthy)
    got = run(e, b.v, b.eps, renorm=True)
    e.close()
    expect = np.where(odd, ST_REPAIRED, 0).astype(np.uint32)
    expect[[3, 8]] = ST_CHOLESKY
    assert np.array_equal(got["status"], expect)
    assert np.array_equal(got["mu"][[3, 8]], bad[[3, 8]]) and np.isnan(got["out_mu"][[3, 8]]).all() and np.isnan(got["eig_min"][[3, 8]]).all()


# ------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(spe):
    b = batch(spe, "pose", "f64", 64)
    e = engine_of(spe, b)
    n = b.n
    lib = spe.load_library()
    vd = dev(e, b.v)
    sent = torch.full((n * e.S,), -7.0, dtype=torch.float64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    p = vd.data_ptr()
    out = spe.ConditionOut(None, None, sent.data_ptr(), None, st.data_ptr())
    good = spe.ConditionIn(p, 1e-10, None, 0)
    for args in ((None, 1e-10, 0), (p, 0.0, 0), (p, 1.0, 0), (p, -1e-4, 0), (p, float("nan"), 0), (p, float("inf"), 0), (p, 1e-10, 2),
                 (p, 1e-10, -1)):   # code 1 = UKFB_ERR_INVALID_ARG
        cin = spe.ConditionIn(args[0], args[1], None, args[2])
        for commit in (0, 1):
            assert lib.ukfb_condition_dev(e._h, C.byref(cin), C.c_int(commit), C.byref(out)) == 1, args
    assert lib.ukfb_condition_dev(e._h, None, C.c_int(1), C.byref(out)) == 1
    assert lib.ukfb_condition_dev(e._h, C.byref(good), C.c_int(0), None) == 1
    assert lib.ukfb_condition_dev(e._h, C.byref(good), C.c_int(0), C.byref(spe.ConditionOut(None, None, None, None, None))) == 1
    assert lib.ukfb_condition_dev(e._h, C.byref(good), C.c_int(2), C.byref(out)) == 1
    assert lib.ukfb_condition_dev(e._h, C.byref(good), C.c_int(-1), C.byref(out)) == 1
    with pytest.raises(spe.UkfbError, match="code 1"):
        e.condition_dev(vd, 1e-10, commit=False)
    # the host form refuses a bad floor before anything is uploaded
    for badv in (0.0, -1.0, float("nan"), float("inf")):
        v = b.v.copy()
        v[4] = badv
        with pytest.raises(spe.UkfbError, match="code 1"):
            e.condition(v, 1e-10)
    with pytest.raises(spe.UkfbError, match="code 1"):
        e.condition(b.v, 1.5)
    torch.cuda.synchronize()
    assert np.array_equal(e.state()[0], b.mu) and np.array_equal(e.state()[1], b.cov) and (e.status() == 0).all()
    assert (sent == -7.0).all() and (st == -1).all()
    e.close()


# ------------------------------------------------------------------------------------------------ 10. host form, all precisions
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_host_array_form(spe, pname):
    """the host form narrows / widens the host doubles itself: its outputs and the committed state are the bits of the device
    form fed the floor rounded to the engine's storage.  Five filters, one of each quarter and a second (b)."""
    big = batch(spe, "pose", pname, 64)
    pick = np.array([int(np.nonzero(big.quarter == q)[0][0]) for q in (1, 0, 2, 3)] + [int(np.nonzero(big.quarter == 1)[0][1])])
    mu, cov = big.mu[pick], big.cov[pick]
    vh = big.v * (1.0 + 1e-9)   # NOT fp32 values
    sel = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    e, twin = engine_of(spe, big, mu=mu, cov=cov), engine_of(spe, big, mu=mu, cov=cov)
    o = e.condition(vh, big.eps, select=sel, renormalize_quaternion=True)
    mu_h, cov_h, _ = e.state()
    d = run(twin, stored(vh, big.dtype), big.eps, select=sel, renorm=True)
    for k, kd in (("eig_min", "eig_min"), ("eig_max", "eig_max"), ("mu", "out_mu"), ("cov", "out_cov"), ("status", "status")):
        assert np.array_equal(o[k], d[kd], equal_nan=True), k
    assert np.array_equal(mu_h, d["mu"]) and np.array_equal(cov_h, d["cov"]) and np.array_equal(e.status(), twin.status())
    assert o["status"][2] == ST_INACTIVE and o["status"][0] == ST_REPAIRED and o["status"][1] in (0, ST_REPAIRED)
    assert not np.array_equal(cov_h[0], cov[0]) and np.array_equal(cov_h[2], cov[2])
    e.close(); twin.close()


# --------------------------------------------------------------------------------------------------------- 11. graph capture
def test_recorded_in_a_graph(spe):
    """condition_dev recorded once in a torch.cuda.graph on the engine's stream and replayed twice: the state and statuses of two
    direct calls on a twin, bit for bit (the second call finds every filter healthy)"""
    b = batch(spe, "pose", "f64", 64)
    n = b.n
    side = torch.cuda.Stream()
    torch.cuda.synchronize()

    def make(stream):
        e = spe.BatchPoseUKF(n, precision=0, stream=stream)
        e.initialize(b.mu, b.cov)
        e.sync()
        return e

    def buffers(e):
        return dev(e, b.v), torch.full((n,), -7.0, dtype=torch.float64, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")

    def round_(e, vd, lo, st):
        e.condition_dev(vd, b.eps, renormalize_quaternion=True, eig_min=lo, status=st)

    twin = make(None)
    tb = buffers(twin)
    for _ in range(2):
        round_(twin, *tb)
    twin.sync()
    torch.cuda.synchronize()
    mu_t, cov_t, _ = twin.state()
    st_t, lo_t = twin.status(), host(tb[1])
    twin.close()

    eng = make(int(side.cuda_stream))
    assert eng.stream_kind == "given"
    gb = buffers(eng)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        round_(eng, *gb)
    torch.cuda.synchronize()
    assert np.array_equal(eng.state()[1], b.cov), "recording must not execute the call"
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    mu_g, cov_g, _ = eng.state()
    assert np.array_equal(mu_g, mu_t) and np.array_equal(cov_g, cov_t) and np.array_equal(eng.status(), st_t)
    assert np.array_equal(host(gb[1]), lo_t) and np.array_equal(gb[2].cpu().numpy().astype(np.uint32), st_t)
    assert (st_t == 0).all() and not np.array_equal(cov_g, b.cov)
    eng.close()


# --------------------------------------------------------------------------------------------------------- 12. device groups
def test_per_shard_through_a_group(spe):
    """a group of two ragged shards on one device, conditioned shard by shard through its engines: the bits of the unsharded batch"""
    b = batch(spe, "pose", "f64", 255)
    base = committed(spe, b)
    grp = spe.UKFGroup(spe.MODEL_POSE, 0, b.n, [0, 0])
    grp.initialize(b.mu, b.cov)
    outs = []
    for sh in grp.shards:
        e = sh["engine"]
        vd = dev(e, b.v)
        st = torch.full((sh["count"],), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        e.condition_dev(vd, b.eps, status=st)
        outs.append(st)
    grp.sync()
    torch.cuda.synchronize()
    mu_g, cov_g, _ = grp.state()
    st_g = np.concatenate([o.cpu().numpy().astype(np.uint32) for o in outs])
    assert [sh["count"] for sh in grp.shards] == [128, 127]
    assert np.array_equal(mu_g, base["mu"]) and np.array_equal(cov_g, base["cov"])
    assert np.array_equal(st_g, base["status"]) and np.array_equal(grp.status(), base["status"])
    grp.close()


# ------------------------------------------------------------------------------------------------------- 13. leftover LDS
def test_no_dependence_on_leftover_lds(spe):
    """the LDS of every compute unit filled with NaN, Inf and zero patterns (tests/cpp/lds_poison.hip, as
    tests/test_gpu_lds_leftovers.py does for the cycle kernels) in front of the call: the same bits -- every LDS scalar the kernel
    reads is one it wrote, the rows that never publish included (wavefronts with failing and unselected rows are in the batch)"""
    poison = lds_poison()
    for model, pname in (("pose", "f64"), ("orient", "f32")):
        b = batch(spe, model, pname, 255)
        sel = (np.arange(b.n) % 7 != 3).astype(np.uint8)
        cov = b.cov.copy()
        cov[21, 2, 1] = cov[21, 1, 2] = np.nan
        runs = []
        for pat in (None,) + LDS_PATTERNS:
            e = engine_of(spe, b, cov=cov)
            if pat is not None:
                torch.cuda.synchronize()
                poison(pat)
            runs.append(run(e, b.v, b.eps, select=sel, renorm=True))
            e.close()
        assert (runs[0]["status"][sel == 0] == ST_INACTIVE).all() and runs[0]["status"][21] == ST_CHOLESKY
        assert (runs[0]["status"] == ST_REPAIRED).sum() > b.n // 2
        for r in runs[1:]:
            assert same(r, runs[0], ALL_KEYS), (model, pname)
