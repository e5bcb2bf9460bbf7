"""User-defined measurement models on the device (ukfb_sigma_points_dev / ukfb_update_sampled_dev and their host forms,
include/ukf_batch.h).

States: those of tests/sensor_meas_cases.py (synth.pose_initial / orient_initial after two real cycles, downloaded and
re-uploaded bit for bit; its `case` cache is shared).  Inputs: tests/sampled_reference.make_inputs (seed 11), rounded to the
engine's storage before the reference sees them.  The samples Z are computed BY THE TEST from the exported X with a torch
expression on the device (tests/sampled_reference.user_h) in the engine's storage type, and the reference takes them as stored.
The reference is tests/sampled_reference.py (pinned by tests/test_sampled_reference.py) run on the state AS DOWNLOADED.  Parity
bound: that of tests/test_gpu_sensor_meas.py, |x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64) / 1e-4 (fp32) / 1e-9 + 2^-23
(wide_arithmetic, against the reference's outputs rounded to fp32).  Every comparison prints a PARITY line before it asserts, and
makes the scaled check of tests/feature_scaled_parity.py (judge_state / judge_meas; plain fp32: margin M_FEAT over the
all-float32 evaluation of tests/sampled_f32.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import feature_scaled_parity as fsp
import sampled_f32 as sf
import sampled_reference as sm
import sensor_meas_cases as smc
import sensor_meas_reference as sr
from engine_support import cycled_engine, dev, host, man_of, same, same_snapshot, scaled, snapshot, stored, tdt
from oracle import ukf_numpy as on

pytestmark = pytest.mark.gpu

N = smc.N   # 1022: not a multiple of four
PRECS = smc.PRECS
ST_NONFINITE, ST_CHOLESKY, ST_UNINIT, ST_INACTIVE, ST_REJECTED = 1 << 4, 1 << 5, 1 << 7, 1 << 8, 1 << 9
OUT_KEYS = ("z_pred", "S", "innov", "maha", "loglik")
ALL_KEYS = ("mu", "cov") + OUT_KEYS + ("status",)


def export(e, want_X=True, want_delta=True):
    """-> (X, delta: device tensors in engine precision or None, status uint32 [n]) after sigma_points_dev"""
    n, dt, pts = e.capacity, tdt(e), 2 * e.D + 1
    X = torch.full((n, pts, e.S), -7.0, dtype=dt, device="cuda") if want_X else None
    dl = torch.full((n, pts, e.D), -7.0, dtype=dt, device="cuda") if want_delta else None
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.sigma_points_dev(X, dl, st)
    e.sync()
    torch.cuda.synchronize()
    return X, dl, st.cpu().numpy().astype(np.uint32)


def run(e, Z, z, Q, active=None, commit=True, q_uniform=False):
    """-> dict(mu, cov, z_pred, S, innov, maha, loglik, status) after update_sampled_dev; Z a device tensor or an array"""
    n, dt = e.capacity, tdt(e)
    Zd = Z if torch.is_tensor(Z) else dev(e, Z)
    m = int(Zd.shape[2])
    zd, qd = dev(e, z), dev(e, np.asarray(Q).reshape(m, m) if q_uniform else np.asarray(Q).reshape(n, m, m))
    ad = None if active is None else torch.from_numpy(np.asarray(active, dtype=np.uint8)).to("cuda")
    o = {"z_pred": torch.full((n, m), -7.0, dtype=dt, device="cuda"), "S": torch.full((n, m, m), -7.0, dtype=dt, device="cuda"),
         "innov": torch.full((n, m), -7.0, dtype=dt, device="cuda"), "maha": torch.full((n,), -7.0, dtype=dt, device="cuda"),
         "loglik": torch.full((n,), -7.0, dtype=dt, device="cuda"), "status": torch.full((n,), -1, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    e.update_sampled_dev(m, Zd.contiguous(), zd, qd, q_is_uniform=q_uniform, active_dev=ad, commit=commit, **o)
    e.sync()
    torch.cuda.synchronize()
    r = {k: host(v) for k, v in o.items() if k != "status"}
    r["status"] = o["status"].cpu().numpy().astype(np.uint32)
    r["mu"], r["cov"], _ = e.state()
    return r


def user(c):
    """the case's user-model inputs (b, r, noise, Q), made once"""
    if not hasattr(c, "user"):
        c.user = sm.make_inputs(c.model, c.mu, c.dtype)
    return c.user


def samples(spe, c, m):
    """-> (Z as stored [n, 2 D + 1, m], z [n, m], Q [n, m, m]) of user model m: Z = h(X) in torch on the device from a fresh
    engine's export, in the engine's storage type; z = h(mu) + noise rounded to it.  Made once per case and m."""
    if not hasattr(c, "samples"):
        c.samples = {}
    if m not in c.samples:
        b, r, noise, Q = user(c)
        e = smc.engine_of(spe, c)
        X, _, st = export(e, want_delta=False)
        assert (st == 0).all()
        Z = host(sm.user_h(c.model, m, X, dev(e, b)[:, None, :], dev(e, r)[:, None, :]))
        e.close()
        z = stored(sm.user_h(c.model, m, c.mu, b, r) + noise[m], c.dtype)
        c.samples[m] = (Z, z, Q[m])
    return c.samples[m]


def reference(c, m, Z, z, Q, gate=-1.0, **kw):
    return sm.update_sampled(man_of(c.model), c.mu, c.cov, Z, z, Q, gate_chi2=gate, **kw)


def check_parity(name, c, got, ref, Z, z, Q, rows=None):
    """the file's bound on every output, then the scaled checks: the updated state block by block, z-bar, S, nu at the scale of S"""
    tol = c.tol
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
    evals = {}

    def f32():
        if not evals:
            for p in ("f32", "f64"):
                evals[p] = sf.update_sampled(c.model, c.mu, c.cov, Z, z, Q, keep=ref["status"] != 0, prec=p)
        return evals
    fsp.judge_state("sampled/" + name, c.model, c.pname, got["mu"][rows], got["cov"][rows], ref["mu"][rows], ref["cov"][rows],
                    f32=lambda: tuple((f32()[p]["mu"][rows], f32()[p]["cov"][rows]) for p in ("f32", "f64")))
    if scored.any():
        pick = lambda o: (o["z_pred"][scored], o["S"][scored], o["innov"][scored])   # noqa: E731
        fsp.judge_meas("sampled/" + name, c.pname, *pick(got), *pick(ref), f32=lambda: tuple(pick(f32()[p]) for p in ("f32", "f64")))


# ------------------------------------------------------------------------------------------------------------------ export
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_export(spe, model, pname):
    c = smc.case(spe, model, pname)
    e = smc.engine_of(spe, c)
    before = snapshot(e)
    X, dl, st = export(e)
    assert same_snapshot(before, snapshot(e))   # read-only on the engine
    Xo, _, st_x = export(e, want_delta=False)
    _, do, st_d = export(e, want_X=False)
    e.close()
    assert (st == 0).all() and (st_x == 0).all() and (st_d == 0).all()
    assert torch.equal(X, Xo) and torch.equal(dl, do)   # either output alone: the same bits
    X, dl = host(X), host(dl)
    assert np.array_equal(X[:, 0], c.mu) and (dl[:, 0] == 0).all()   # point 0 is mu bit for bit
    Xr, dr, sr_ = sm.sigma_points(man_of(model), c.mu, c.cov)
    assert (sr_ == 0).all()
    if c.wide:
        Xr, dr = stored(Xr, np.float32), stored(dr, np.float32)
    ex, ed = scaled(X, Xr), scaled(dl, dr)
    print(f"PARITY export {model}/{pname} n={c.n} max_scaled_dX={ex:.3e} max_scaled_ddelta={ed:.3e} tol={c.tol:.3e}")
    assert ex <= c.tol and ed <= c.tol
    assert np.array_equal(dl[:, 1::2], -dl[:, 2::2])


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_export_failures_stay_inside_their_filter(spe, model):
    """an uninitialised filter and one whose covariance does not factorise: rows of NaN and their status; the wave-mates keep
    the bits of a run without the broken covariance"""
    n, dead, neg = 64, 22, 34
    man = man_of(model)
    e = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    mu, cov, init = e.state()
    assert not init[dead]
    Xc, dc, stc = export(e)
    assert np.array_equal(stc, np.where(np.arange(n) == dead, ST_UNINIT, 0))
    e.initialize(mu[neg:neg + 1], -np.eye(man.D)[None], first=neg)
    X, dl, st = export(e)
    e.close()
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[neg] = ST_UNINIT, ST_CHOLESKY
    assert np.array_equal(st, expect)
    X, dl, Xc, dc = host(X), host(dl), host(Xc), host(dc)
    bad = expect != 0
    assert np.isnan(X[bad]).all() and np.isnan(dl[bad]).all() and np.isnan(Xc[dead]).all() and np.isnan(dc[dead]).all()
    assert np.array_equal(X[~bad], Xc[~bad]) and np.array_equal(dl[~bad], dc[~bad]) and np.isfinite(X[~bad]).all()
    cov_bad = cov.copy()
    cov_bad[neg] = -np.eye(man.D)
    assert np.array_equal(sm.sigma_points(man, mu, cov_bad, initialised=init)[2], expect)


# ------------------------------------------------------------------------------------------------------------------ parity
_RUNS = {}


def committed(spe, c, m):
    """the committing run of user model m on a fresh engine of the case, made once"""
    key = (c.model, c.pname, c.n, m)
    if key not in _RUNS:
        Z, z, Q = samples(spe, c, m)
        e = smc.engine_of(spe, c)
        _RUNS[key] = run(e, Z, z, Q)
        assert np.array_equal(e.status(), _RUNS[key]["status"])   # commit = 1 writes the engine's own status array too
        e.close()
    return _RUNS[key]


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_parity(spe, model, pname):
    c = smc.case(spe, model, pname)
    for m in sm.USER_DIMS:
        Z, z, Q = samples(spe, c, m)
        got, ref = committed(spe, c, m), reference(c, m, Z, z, Q)
        assert (ref["status"] == 0).all(), (m, np.unique(ref["status"]))
        assert (got["status"] == 0).all(), (m, np.unique(got["status"]))
        check_parity(f"{model}/{pname}/m={m}", c, got, ref, Z, z, Q)
        assert not np.array_equal(got["mu"], c.mu)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_small_batches(spe, model):
    """1, 2, 3 and 5 filters: one partly filled wavefront, and a full one with a one-row tail"""
    big = smc.case(spe, model, "f64", 255)
    for n in (1, 2, 3, 5):
        c = smc.Case()
        c.model, c.pname, c.n, c.prec, c.wide, c.tol, c.dtype = model, "f64", n, 0, 0, 1e-9, big.dtype
        c.mu, c.cov, c.gyro = big.mu[:n], big.cov[:n], big.gyro[:n]
        for m in (1, 6):
            Z, z, Q = samples(spe, c, m)
            got, ref = committed(spe, c, m), reference(c, m, Z, z, Q)
            assert (got["status"] == 0).all() and (ref["status"] == 0).all()
            check_parity(f"{model}/f64/m={m}/n={n}", c, got, ref, Z, z, Q)


# --------------------------------------------------------------------------------------------- a user model = a built-in one
def test_user_model_reproduces_builtin(spe):
    """fp64 only: X is exported, Z formed in torch with the formula of a built-in model, and update_sampled_dev and the built-in
    call on a twin engine are each within tol of the same reference.  Storage precisions are left out: the built-in kernels
    evaluate h on sigma points they hold in fp64 registers, a user model sees X rounded to fp32 -- an input perturbation, not a
    kernel error."""
    for model, mid in (("pose", sr.POSE_RANGE), ("pose", sr.POSE_POINT), ("orient", sr.ORIENT_NAV_VECTOR)):
        c = smc.case(spe, model, "f64")
        m = sr.meas_dim(mid)
        e, twin = smc.engine_of(spe, c), smc.engine_of(spe, c)
        X, _, _ = export(e)
        r, qs, b = dev(e, c.mount[:, None, 0:3]), dev(e, c.mount[:, None, 3:7]), dev(e, c.point[:, None, :])
        if mid == sr.POSE_RANGE:
            Zt = sm._norm((X[..., 0:3] - b) + sm.rot(X[..., 3:7], r))
        elif mid == sr.POSE_POINT:
            Zt = sm.rot_t(qs, sm.rot_t(X[..., 3:7], b - X[..., 0:3]) - r)
        else:
            Zt = sm.rot_t(qs, sm.rot_t(X[..., 0:4], b + 0.0 * X[..., 4:7]))
        got = run(e, Zt, c.z[mid][:, :m], c.Q[:, :m, :m])
        built = smc.run_case(twin, c, mid)
        e.close(); twin.close()
        ref = smc.reference(c, mid)
        assert (got["status"] == 0).all() and (built["status"] == 0).all() and (ref["status"] == 0).all()
        cut = {"z_pred": ref["z_pred"][:, :m], "S": ref["S"][:, :m, :m], "innov": ref["innov"][:, :m]}
        err = {k: scaled(got[k], cut.get(k, ref[k])) for k in ALL_KEYS[:-1]}
        err_b = {k: scaled(built[k], ref[k]) for k in ALL_KEYS[:-1]}
        print(f"PARITY sampled-as-{sr.NAMES[mid]} n={c.n} " + " ".join(f"d{k}={v:.3e}" for k, v in err.items()) +
              f" built-in worst={max(err_b.values()):.3e} tol={c.tol:.3e}")
        assert all(v <= c.tol for v in err.values()) and all(v <= c.tol for v in err_b.values()), (mid, err, err_b)
    # the position selection against ukfb_update_dev(UKFB_MEAS_POS3)
    c = smc.case(spe, "pose", "f64")
    z = stored(c.mu[:, 0:3] + 0.05 * np.random.default_rng(29).standard_normal((c.n, 3)), c.dtype)
    e, twin = smc.engine_of(spe, c), smc.engine_of(spe, c)
    X, _, _ = export(e)
    got = run(e, X[..., 0:3], z, c.Q)
    twin.update(spe.MEAS_POS3, z, c.Q)
    mu_t, cov_t, _ = twin.state()
    assert (got["status"] == 0).all() and twin.status_summary() == 0
    e.close(); twin.close()
    mu_r, cov_r, st_r = on.pose_update(c.mu, c.cov, on.MEAS_POS3, z, c.Q)
    assert (st_r == 0).all()
    errs = (scaled(got["mu"], mu_r), scaled(got["cov"], cov_r), scaled(mu_t, mu_r), scaled(cov_t, cov_r))
    print(f"PARITY sampled-as-POS3 n={c.n} dmu={errs[0]:.3e} dcov={errs[1]:.3e} update_dev dmu={errs[2]:.3e} dcov={errs[3]:.3e} tol={c.tol:.3e}")
    assert all(v <= c.tol for v in errs), errs


# ------------------------------------------------------------------------------------------------------- bit-level properties
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_bit_level_properties(spe, model):
    c = smc.case(spe, model, "f64")
    n, m = c.n, 4
    Z, z, Q = samples(spe, c, m)
    base = committed(spe, c, m)
    assert (base["status"] == 0).all()

    def fresh(**kw):
        e = smc.engine_of(spe, c, **kw)
        e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
        return e
    # commit = 0: the whole downloadable engine keeps its bits, the outputs are the committing call's; then commit = 1: the
    # numbers of commit = 1 alone
    e = fresh()
    before = snapshot(e)
    dry = run(e, Z, z, Q, commit=False)
    assert same_snapshot(before, snapshot(e))
    assert same(dry, base, OUT_KEYS + ("status",)) and np.array_equal(dry["mu"], c.mu) and np.array_equal(dry["cov"], c.cov)
    assert same(run(e, Z, z, Q), base, ALL_KEYS)
    e.close()
    # active = NULL equals all ones; a gate nothing reaches = no gate
    e = fresh(gate_chi2=1e300)
    assert same(run(e, Z, z, Q, active=np.ones(n, dtype=np.uint8)), base, ALL_KEYS)
    e.close()
    # ONE m x m with q_is_uniform equals the repeated Q
    Qu = np.broadcast_to(Q[5], Q.shape).copy()
    e, e2 = fresh(), fresh()
    assert same(run(e, Z, z, Qu[0], q_uniform=True), run(e2, Z, z, Qu), ALL_KEYS)
    e.close(); e2.close()
    # a filter's bits are the same in the batch of 1022, alone, and at another index (row 2 of a second wavefront)
    i = 7
    for nn, at in ((1, 0), (7, 6)):
        s = smc.Case()
        s.__dict__.update(c.__dict__)
        s.n = nn
        pick = np.arange(nn) + 40   # the other rows: other filters' states
        pick[at] = i
        s.mu, s.cov, s.gyro = c.mu[pick], c.cov[pick], c.gyro[pick]
        e = smc.engine_of(spe, s)
        one = run(e, Z[pick], z[pick], Q[pick])
        e.close()
        assert all(np.array_equal(one[k][at], base[k][i], equal_nan=True) for k in ALL_KEYS), (nn, at)
    # translation: samples and z on a 2^-20 grid, a per-filter translation on that grid up to 1000 -- every sum Z + t is then
    # exact in fp64, so that the differences the kernel forms first are the same bits: mean, covariance, S, nu, d^2 and the
    # log-likelihood keep every bit, z-bar moves by the translation
    grid = lambda x: np.round(np.asarray(x) * 2.0 ** 20) / 2.0 ** 20   # noqa: E731
    Zg, zg = grid(Z), grid(z)
    t = grid(np.random.default_rng(3).uniform(-1000.0, 1000.0, (n, m)))
    e, e2 = fresh(), fresh()
    a, b = run(e, Zg, zg, Q), run(e2, Zg + t[:, None, :], zg + t, Q)
    e.close(); e2.close()
    assert (a["status"] == 0).all() and same(a, b, ("mu", "cov", "S", "innov", "maha", "loglik", "status"))
    assert np.abs(b["z_pred"] - (a["z_pred"] + t)).max() <= 1e-12 * 1000.0


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", ["f64", "f32"])
def test_gate(spe, model, pname):
    """gate_chi2 = the median of the reference's d^2: accepted and REJECTED_GATE split as the reference's; filters within the
    margin of tests/test_gpu_sensor_meas.py::test_gate of the gate are left out, under its cap"""
    c = smc.case(spe, model, pname)
    m = 3
    Z, z, Q = samples(spe, c, m)
    free = reference(c, m, Z, z, Q)
    gate = float(np.median(free["maha"]))
    assert free["maha"].min() < gate < free["maha"].max()
    ref = reference(c, m, Z, z, Q, gate=gate)
    e = smc.engine_of(spe, c, gate_chi2=gate)
    got = run(e, Z, z, Q)
    e.close()
    near = np.abs(free["maha"] - gate) <= c.tol * (1.0 + free["maha"])
    assert near.sum() <= c.n // 100, int(near.sum())
    rows = ~near
    assert np.array_equal(got["status"][rows], ref["status"][rows])
    rej = rows & (ref["status"] == ST_REJECTED)
    assert rej.sum() > c.n // 4 and (rows & (ref["status"] == 0)).sum() > c.n // 4
    assert np.array_equal(got["mu"][rej], c.mu[rej]) and np.array_equal(got["cov"][rej], c.cov[rej])
    assert np.isfinite(got["maha"][rej]).all()
    check_parity(f"{model}/{pname}/gate", c, got, ref, Z, z, Q, rows=rows)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failures_stay_inside_their_filter(spe, model):
    """One NaN among the (2 D + 1) m samples, a NaN in z, a Q with a negative pivot, an uninitialised filter, active = 0: each in
    a wavefront with three healthy filters, which keep the bits of a clean run; a NaN in Q's upper triangle changes nothing"""
    n, m, dead = 64, 6, 22
    nan_s, nan_z, neg_q, idle, upper = 13, 17, 25, 38, 41   # every one in another wavefront
    man = man_of(model)
    e = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    mu, cov, init = e.state()
    assert not init[dead] and init.sum() == n - 1
    mu_f = mu.copy()
    mu_f[dead] = mu[0]
    b, r, noise, Qs = sm.make_inputs(model, mu_f, np.float64)
    X, _, st = export(e)
    assert np.array_equal(st, np.where(np.arange(n) == dead, ST_UNINIT, 0))
    Z = host(sm.user_h(model, m, X, dev(e, b)[:, None, :], dev(e, r)[:, None, :]))
    Z[dead] = 0.0   # (its exported rows are NaN; the update must report UNINITIALISED whatever the samples are)
    z, Q = sm.user_h(model, m, mu_f, b, r) + noise[m], Qs[m]
    clean = run(e, Z, z, Q, commit=False)
    assert np.array_equal(clean["status"], np.where(np.arange(n) == dead, ST_UNINIT, 0))
    Zb, zb, Qb, act = Z.copy(), z.copy(), Q.copy(), np.ones(n, dtype=np.uint8)
    Zb[nan_s, 2 * man.D, m - 1] = np.nan   # the last sample of the record
    zb[nan_z, 1] = np.nan
    Qb[neg_q] = -1e6 * np.eye(m)
    Qb[upper, 0, m - 1] = np.nan
    act[idle] = 0
    got = run(e, Zb, zb, Qb, active=act)
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[neg_q], expect[idle] = ST_UNINIT, ST_CHOLESKY, ST_INACTIVE
    expect[[nan_s, nan_z]] = ST_NONFINITE
    assert np.array_equal(got["status"], expect), (got["status"], expect)
    assert np.array_equal(e.status(), expect)
    e.close()
    failing = expect != 0
    assert np.array_equal(got["mu"][failing], mu[failing], equal_nan=True) and np.array_equal(got["cov"][failing], cov[failing], equal_nan=True)
    assert all(np.isnan(got[k][failing]).all() for k in OUT_KEYS)
    twin = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    ok = run(twin, Z, z, Q)
    twin.close()
    assert same(ok, clean, OUT_KEYS + ("status",))
    assert same(got, ok, ALL_KEYS, rows=~failing)
    assert not np.array_equal(got["mu"][upper], mu[upper])
    ref = sm.update_sampled(man, mu_f, cov, Zb, zb, Qb, active=act, initialised=init)
    assert np.array_equal(ref["status"], expect)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(spe):
    c = smc.case(spe, "pose", "f64", 255)
    e = smc.engine_of(spe, c)
    n, pts = c.n, 2 * e.D + 1
    for m in (0, 7):   # code 4 = UKFB_ERR_OUT_OF_RANGE; nothing is written
        Zd = torch.zeros((n, pts, max(m, 1)), dtype=torch.float64, device="cuda")
        zd = torch.zeros((n, max(m, 1)), dtype=torch.float64, device="cuda")
        qd = torch.ones((n, max(m, 1) ** 2), dtype=torch.float64, device="cuda")
        out = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        with pytest.raises(spe.UkfbError, match="code 4"):
            e.update_sampled_dev(m, Zd, zd, qd, maha=out, status=st)
        torch.cuda.synchronize()
        assert (out == -7.0).all() and (st == -1).all()
    lib = spe.load_library()
    buf = torch.zeros(n * pts * 6, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    out = spe.SampledOut(None, None, None, p, None, None)
    for args in ((None, p, p), (p, None, p), (p, p, None)):   # code 1 = UKFB_ERR_INVALID_ARG
        sin = spe.SampledIn(3, args[0], args[1], args[2], 0, None)
        assert lib.ukfb_update_sampled_dev(e._h, C.byref(sin), C.c_int(1), C.byref(out)) == 1
    sin = spe.SampledIn(3, p, p, p, 0, None)
    assert lib.ukfb_update_sampled_dev(e._h, None, C.c_int(1), C.byref(out)) == 1
    assert lib.ukfb_update_sampled_dev(e._h, C.byref(sin), C.c_int(0), None) == 1
    assert lib.ukfb_update_sampled_dev(e._h, C.byref(sin), C.c_int(0), C.byref(spe.SampledOut(None, None, None, None, None, None))) == 1
    assert lib.ukfb_update_sampled_dev(e._h, C.byref(sin), C.c_int(2), C.byref(out)) == 1
    assert lib.ukfb_sigma_points_dev(e._h, None, None, None) == 1
    torch.cuda.synchronize()
    assert np.array_equal(e.state()[0], c.mu) and np.array_equal(e.state()[1], c.cov) and (buf == 0).all()
    e.close()


@pytest.mark.parametrize("pname", ["f32", "f32w"])
def test_host_array_form_fp32(spe, pname):
    """fp32 engines: the host forms narrow / widen the host doubles themselves; their outputs and the committed state are the
    bits of the device forms fed the same values rounded to float32.  Five filters."""
    n, m = 5, 3
    c = smc.case(spe, "pose", pname, n)
    b, r, noise, Qs = user(c)
    e, twin = smc.engine_of(spe, c), smc.engine_of(spe, c)
    X, dl, st = e.sigma_points()
    Xd, dd, std = export(twin)
    assert np.array_equal(X, host(Xd)) and np.array_equal(dl, host(dd)) and np.array_equal(st, std) and (st == 0).all()
    rng = np.random.default_rng(9)
    Z = sm.user_h("pose", m, X, b[:, None, :], r[:, None, :]) + 1e-9 * rng.standard_normal((n, 2 * e.D + 1, m))   # NOT fp32 values
    z = sm.user_h("pose", m, c.mu, b, r) + noise[m]
    assert not np.array_equal(Z, stored(Z, np.float32))
    o = e.update_sampled(Z, z, Qs[m])
    o["mu"], o["cov"], _ = e.state()
    d = run(twin, stored(Z, np.float32), stored(z, np.float32), Qs[m])
    assert same(o, d, ALL_KEYS) and np.array_equal(e.status(), twin.status()) and (o["status"] == 0).all()
    e.close(); twin.close()
