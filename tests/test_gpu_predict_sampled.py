"""User-defined process models on the device (ukfb_predict_sampled_dev and its host form, include/ukf_batch.h).

States: those of tests/sensor_meas_cases.py (synth.pose_initial / orient_initial after two real cycles, downloaded and
re-uploaded bit for bit; its `case` cache is shared).  Inputs: tests/predict_sampled_reference.make_inputs (seed 17), rounded to
the engine's storage before the reference sees them.  The propagated points XX are computed BY THE TEST from the exported X with
a torch expression on the device (tests/predict_sampled_reference.user_f) in the engine's storage type, and the reference takes
them and R as stored.  The reference is tests/predict_sampled_reference.py (pinned by tests/test_predict_sampled_reference.py)
run on the state AS DOWNLOADED.  Parity bound: that of tests/test_gpu_sampled.py, |x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64)
/ 1e-4 (fp32) / 1e-9 + 2^-23 (wide_arithmetic, against the reference's outputs rounded to fp32).  Every comparison prints a
PARITY line before it asserts, and makes the scaled check of tests/feature_scaled_parity.py (judge_state; plain fp32: margin
M_FEAT over the all-float32 evaluation of tests/predict_sampled_f32.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import feature_scaled_parity as fsp
import predict_sampled_f32 as pf
import predict_sampled_reference as pr
import sampled_reference as sm
import sensor_meas_cases as smc
from engine_support import (ACC_COV, cycled_engine, dev, host, man_of, same, same_snapshot, scaled, snapshot, stored, tdt,
                            unpack)
from oracle import ukf_numpy as on

pytestmark = pytest.mark.gpu

N = smc.N   # 1022: not a multiple of four
PRECS = smc.PRECS
ST_NONFINITE, ST_CHOLESKY, ST_NOCONV, ST_UNINIT, ST_INACTIVE = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8
ALL_KEYS = ("mu", "cov", "out_mu", "out_cov", "status")


def export(e):
    """-> (X: a device tensor in engine precision, status uint32 [n]) after sigma_points_dev"""
    X = torch.full((e.capacity, 2 * e.D + 1, e.S), -7.0, dtype=tdt(e), device="cuda")
    st = torch.full((e.capacity,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.sigma_points_dev(X, None, st)
    e.sync()
    torch.cuda.synchronize()
    return X, st.cpu().numpy().astype(np.uint32)


def run(e, XX, R, active=None, commit=True, r_uniform=False, outs=True):
    """-> dict(mu, cov: the engine's state after the call; out_mu, out_cov, status: the call's outputs) after
    predict_sampled_dev; XX a device tensor or an array"""
    n, dt, D = e.capacity, tdt(e), e.D
    Xd = XX if torch.is_tensor(XX) else dev(e, XX)
    Rd = dev(e, np.asarray(R).reshape(D, D) if r_uniform else np.asarray(R).reshape(n, D, D))
    ad = None if active is None else torch.from_numpy(np.asarray(active, dtype=np.uint8)).to("cuda")
    o = {}
    if outs:
        o = {"mu": torch.full((n, e.S), -7.0, dtype=dt, device="cuda"), "cov_packed": torch.full((n, D * (D + 1) // 2), -7.0, dtype=dt, device="cuda"),
             "status": torch.full((n,), -1, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    e.predict_sampled_dev(Xd.contiguous(), Rd, r_is_uniform=r_uniform, active_dev=ad, commit=commit, **o)
    e.sync()
    torch.cuda.synchronize()
    r = {}
    if outs:
        r = {"out_mu": host(o["mu"]), "out_cov": unpack(host(o["cov_packed"]), D), "status": o["status"].cpu().numpy().astype(np.uint32)}
    r["mu"], r["cov"], _ = e.state()
    return r


def user(c):
    """the case's user-model inputs (parameters per model, R), made once"""
    if not hasattr(c, "puser"):
        c.puser = pr.make_inputs(c.model, c.mu, c.dtype)
    return c.puser


def propagate(e, model, name, par, X, dt=pr.DT):
    """XX = f(X) in torch on the device, in the engine's storage type"""
    return pr.user_f(model, name, X, {k: dev(e, v) for k, v in pr.expand(par).items()}, dt=dt)


def samples(spe, c, name):
    """-> (XX as stored [n, 2 D + 1, S], R [n, D, D]) of user model `name`, from a fresh engine's export; made once per case"""
    if not hasattr(c, "psamples"):
        c.psamples = {}
    if name not in c.psamples:
        par, R = user(c)
        e = smc.engine_of(spe, c)
        X, st = export(e)
        assert (st == 0).all()
        if name == "wide":
            XX = propagate(e, c.model, "turn", pr.wide_turn(par["turn"]), X, dt=pr.WIDE_TURN_DT)
        else:
            XX = propagate(e, c.model, name, par[name], X)
        e.close()
        c.psamples[name] = (host(XX), R)
    return c.psamples[name]


def reference(c, XX, R, **kw):
    return pr.predict_sampled(man_of(c.model), c.mu, c.cov, XX, R, **kw)


def check_parity(name, c, got, ref, XX, R, rows=None):
    """the file's bound on the committed state and on the call's outputs, then the scaled check of the state block by block"""
    tol = c.tol
    rows = np.ones(c.n, bool) if rows is None else rows
    r = {k: np.asarray(ref[k], dtype=np.float64) for k in ("mu", "cov")}
    if c.wide:   # the engine stores fp32
        r = {k: v.astype(np.float32).astype(np.float64) for k, v in r.items()}
    err = {k: scaled(got[k][rows], r[k][rows]) for k in ("mu", "cov")}
    print(f"PARITY predict_sampled {name} n={int(rows.sum())} " + " ".join(f"max_scaled_d{k}={v:.3e}" for k, v in err.items()) + f" tol={tol:.3e}")
    assert all(v <= tol for v in err.values()), (name, err, tol)
    if "out_mu" in got:   # the call's own outputs are the committed numbers
        assert np.array_equal(got["out_mu"][rows], got["mu"][rows]) and np.array_equal(got["out_cov"][rows], got["cov"][rows])
    evals = {}

    def f32():
        if not evals:
            for p in ("f32", "f64"):
                evals[p] = pf.predict_sampled(c.model, c.mu, c.cov, XX, R, keep=(ref["status"] & ~np.uint32(ST_NOCONV)) != 0, prec=p)
        return evals
    fsp.judge_state("predict_sampled/" + name, c.model, c.pname, got["mu"][rows], got["cov"][rows], ref["mu"][rows], ref["cov"][rows],
                    f32=lambda: tuple((f32()[p]["mu"][rows], f32()[p]["cov"][rows]) for p in ("f32", "f64")))


_RUNS = {}


def committed(spe, c, name):
    """the committing run of user model `name` on a fresh engine of the case, made once"""
    key = (c.model, c.pname, c.n, name)
    if key not in _RUNS:
        XX, R = samples(spe, c, name)
        e = smc.engine_of(spe, c)
        _RUNS[key] = run(e, XX, R)
        assert np.array_equal(e.status(), _RUNS[key]["status"])   # commit = 1 writes the engine's own status array too
        e.close()
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_parity(spe, model, pname):
    c = smc.case(spe, model, pname)
    for name in pr.USER_MODELS[model]:
        XX, R = samples(spe, c, name)
        got, ref = committed(spe, c, name), reference(c, XX, R)
        assert (ref["status"] == 0).all(), (name, np.unique(ref["status"]))
        assert (got["status"] == 0).all(), (name, np.unique(got["status"]))
        check_parity(f"{model}/{pname}/{name}", c, got, ref, XX, R)
        assert not np.array_equal(got["mu"], c.mu) and not np.array_equal(got["cov"], c.cov)


# --------------------------------------------------------------------------------------------- 2. a user model = a built-in one
def test_user_model_reproduces_builtin(spe):
    """fp64 only: X is exported, XX formed in torch with the formula of a built-in process model, R formed as the oracle forms it
    (rotated blocks, dt or dt^2 scaling, the acceleration block), and predict_sampled_dev and ukfb_predict on a twin engine are
    each within tol of on.pose_predict / on.orient_predict.  Storage precisions are left out: the built-in kernels propagate
    sigma points they hold in fp64 registers, a user model sees X rounded to fp32 -- an input perturbation, not a kernel error."""
    sy, dt = spe.synth, 0.01
    for model, with_acc in (("pose", True), ("pose", False), ("orient", True)):
        c = smc.case(spe, model, "f64")
        n = c.n
        e, twin = smc.engine_of(spe, c), smc.engine_of(spe, c)
        X, st = export(e)
        assert (st == 0).all()
        if model == "pose":
            Rn = np.broadcast_to(sy.pose_default_process_noise(), (n, 12, 12))
            acc = sy.pose_cycle_inputs(n, 2, c.mu[:, :3])[0] if with_acc else None
            XX = pr.pose_builtin(X, None if acc is None else dev(e, acc)[:, None, :], dt)
            R = Rn.copy()
            if with_acc:
                R[:, 6:9, 6:9] = 2.0 * ACC_COV
                twin.set_acceleration(acc, ACC_COV)
            else:
                rot = on.quat_to_matrix(c.mu[:, 3:7])
                R[:, 0:3, 0:3], R[:, 3:6, 3:6] = on._rotate_block(rot, Rn, 0), on._rotate_block(rot, Rn, 3)
                R = dt * R
            ref = on.pose_predict(c.mu, c.cov, sy.pose_default_process_noise(), acc, ACC_COV, dt)
        else:
            earth = on.earth_rotation(sy.ORIENT_LATITUDE)
            gyro, acc, _, _ = sy.orient_cycle_inputs(n, 2, c.mu[:, 0:4])
            XX = pr.orient_builtin(X, dev(e, acc)[:, None, :], dev(e, gyro)[:, None, :], -1.0 / sy.ORIENT_TAU, -1.0 / sy.ORIENT_TAU,
                                   dev(e, earth)[None, None, :], dt)
            Rn = np.broadcast_to(sy.orient_process_noise(), (n, 13, 13))
            rot = on.quat_to_matrix(c.mu[:, 0:4])
            R = Rn.copy()
            R[:, 0:3, 0:3], R[:, 3:6, 3:6] = on._rotate_block(rot, Rn, 0), on._rotate_block(rot, Rn, 3)
            R = dt ** 2 * R
            twin.set_orient_inputs(gyro, acc)
            ref = on.orient_predict(c.mu, c.cov, sy.orient_process_noise(), acc, gyro, sy.ORIENT_TAU, sy.ORIENT_TAU, earth, dt)
        got = run(e, XX, R)
        twin.predict(dt)
        mu_t, cov_t, _ = twin.state()
        assert (got["status"] == 0).all() and twin.status_summary() == 0 and (ref[2] == 0).all()
        e.close(); twin.close()
        errs = (scaled(got["mu"], ref[0]), scaled(got["cov"], ref[1]), scaled(mu_t, ref[0]), scaled(cov_t, ref[1]))
        print(f"PARITY predict_sampled-as-{model}{'+acc' if with_acc and model == 'pose' else ''} n={n} dmu={errs[0]:.3e} "
              f"dcov={errs[1]:.3e} ukfb_predict dmu={errs[2]:.3e} dcov={errs[3]:.3e} tol={c.tol:.3e}")
        assert all(v <= c.tol for v in errs), errs
        assert not np.array_equal(got["mu"], c.mu)


# ----------------------------------------------------------------------------------------------------------- 3. small batches
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_small_batches(spe, model):
    """1, 2, 3 and 5 filters: one partly filled wavefront, and a full one with a one-row tail"""
    big = smc.case(spe, model, "f64", 255)
    for n in (1, 2, 3, 5):
        c = smc.Case()
        c.model, c.pname, c.n, c.prec, c.wide, c.tol, c.dtype = model, "f64", n, 0, 0, 1e-9, big.dtype
        c.mu, c.cov, c.gyro = big.mu[:n], big.cov[:n], big.gyro[:n]
        name = pr.USER_MODELS[model][-1]
        XX, R = samples(spe, c, name)
        got, ref = committed(spe, c, name), reference(c, XX, R)
        assert (got["status"] == 0).all() and (ref["status"] == 0).all()
        check_parity(f"{model}/f64/{name}/n={n}", c, got, ref, XX, R)


# ----------------------------------------------------------------------------------------------- 4. several mean iterations
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_several_mean_iterations(spe, pname):
    """a coordinated turn whose rate x dt spreads the propagated orientations by radians (predict_sampled_reference.wide_turn
    says why ~ 1 rad is not enough): the reference needs more than two trips for most filters"""
    c = smc.case(spe, "pose", pname)
    XX, R = samples(spe, c, "wide")
    trips = pr.mean_trips(on.POSE, XX)   # on the CPU, before the GPU is asked
    spread = np.linalg.norm(on.POSE.boxminus(XX, XX[:, 0:1])[..., 3:6], axis=-1).max(axis=1)
    print(f"PARITY predict_sampled wide/{pname} trips={np.bincount(trips).tolist()} spread median={np.median(spread):.3f} max={spread.max():.3f}")
    assert (trips > 2).mean() > 0.5 and np.median(spread) > 1.0 and spread.max() < 3.0
    got, ref = committed(spe, c, "wide"), reference(c, XX, R)
    assert (ref["status"] == 0).all() and (got["status"] == 0).all()
    check_parity(f"pose/{pname}/wide", c, got, ref, XX, R)
    if pname != "f64":
        return
    # mean_max_iter = 1: the filters that still move after their first trip, every one of them
    capped = reference(c, XX, R, max_it=1)
    e = smc.engine_of(spe, c, mean_max_iter=1)
    one = run(e, XX, R)
    e.close()
    assert set(np.unique(capped["status"])) <= {0, ST_NOCONV} and (capped["status"] == ST_NOCONV).sum() > c.n // 2
    assert np.array_equal(one["status"], capped["status"])
    check_parity("pose/f64/wide/max_it=1", c, one, capped, XX, R)


# ------------------------------------------------------------------------------------------------- 5. bit-level properties
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_bit_level_properties(spe, model):
    c = smc.case(spe, model, "f64")
    n, name = c.n, pr.USER_MODELS[model][0]
    XX, R = samples(spe, c, name)
    base = committed(spe, c, name)
    assert (base["status"] == 0).all()
    stamps = np.arange(1, n + 1, dtype=np.int64) * 1000 + 7

    def fresh(**kw):
        e = smc.engine_of(spe, c, **kw)
        e.set_last_measurement_time(stamps)
        return e
    # commit = 0: the whole downloadable engine keeps its bits, the outputs are the committing call's; then commit = 1 without
    # `out`: the numbers of commit = 1 with it; the stamps set before the calls are the stamps after them
    e = fresh()
    before = snapshot(e)
    dry = run(e, XX, R, commit=False)
    assert same_snapshot(before, snapshot(e))
    assert same(dry, base, ("out_mu", "out_cov", "status")) and np.array_equal(dry["mu"], c.mu) and np.array_equal(dry["cov"], c.cov)
    alone = run(e, XX, R, outs=False)
    assert same(alone, base, ("mu", "cov")) and np.array_equal(e.status(), base["status"])
    assert np.array_equal(e.last_measurement_time(), stamps)
    after = snapshot(e)
    # times and noise tables (the rotation rate of the snapshot is a function of the committed bias: it may move)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before[4:6], after[4:6]))
    e.close()
    # active = NULL equals all ones
    e = fresh()
    assert same(run(e, XX, R, active=np.ones(n, dtype=np.uint8)), base, ALL_KEYS)
    e.close()
    # ONE D x D with r_is_uniform equals the repeated R
    Ru = np.broadcast_to(R[5], R.shape).copy()
    e, e2 = fresh(), fresh()
    assert same(run(e, XX, Ru[0], r_uniform=True), run(e2, XX, Ru), ALL_KEYS)
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
        one = run(e, XX[pick], R[pick])
        e.close()
        assert all(np.array_equal(one[k][at], base[k][i], equal_nan=True) for k in ALL_KEYS), (nn, at)
    # translation: the points on a 2^-20 grid, a per-filter translation on that grid up to 1000 added to the position block (the
    # OrientationState's velocity block) of every point -- every sum is then exact in fp64, so that the differences the kernel
    # forms first are the same bits: covariance, quaternion and the other vector blocks keep every bit, the block's mean moves
    grid = lambda x: np.round(np.asarray(x) * 2.0 ** 20) / 2.0 ** 20   # noqa: E731
    sl = slice(0, 3) if model == "pose" else slice(4, 7)
    others = np.ones(c.mu.shape[1], bool)
    others[sl] = False
    XXg = grid(XX)
    t = grid(np.random.default_rng(3).uniform(-1000.0, 1000.0, (n, 3)))
    XXt = XXg.copy()
    XXt[:, :, sl] += t[:, None, :]
    e, e2 = fresh(), fresh()
    a, b = run(e, XXg, R), run(e2, XXt, R)
    e.close(); e2.close()
    assert (a["status"] == 0).all() and same(a, b, ("cov", "out_cov", "status"))
    assert np.array_equal(a["mu"][:, others], b["mu"][:, others])
    d = np.abs(b["mu"][:, sl] - (a["mu"][:, sl] + t)).max()
    print(f"PARITY predict_sampled translation {model} n={n} max |mean moved - translation| = {d:.3e} bound={1e-12 * 1000.0:.3e}")
    assert d <= 1e-12 * 1000.0


# ------------------------------------------------------------------------------------- 6. failures stay inside their filter
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failures_stay_inside_their_filter(spe, model):
    """A NaN in the last scalar of the sample record, a NaN in R's lower triangle, active = 0, an uninitialised filter whose
    samples are finite, a filter whose covariance is -I (its exported rows are NaN): each in a wavefront with three healthy
    filters, which keep the bits of a clean twin; a NaN in R's upper triangle changes nothing"""
    n, dead = 64, 22
    nan_s, nan_r, neg, idle, upper = 13, 17, 34, 38, 41   # every one in another wavefront
    man = man_of(model)
    name = pr.USER_MODELS[model][0]

    def make():
        e = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
        mu, cov, init = e.state()
        mu_f = mu.copy()
        mu_f[dead] = mu[0]
        par, R = pr.make_inputs(model, mu_f, np.float64)
        return e, mu, cov, init, par, R
    twin, mu, cov, init, par, R = make()
    assert not init[dead] and init.sum() == n - 1
    Xc, st = export(twin)
    assert np.array_equal(st, np.where(np.arange(n) == dead, ST_UNINIT, 0))
    XXc = host(propagate(twin, model, name, par[name], Xc))
    XXc[dead] = XXc[0]   # (its exported rows are NaN; the call must report UNINITIALISED whatever the samples are)
    clean = run(twin, XXc, R)
    twin.close()
    assert np.array_equal(clean["status"], np.where(np.arange(n) == dead, ST_UNINIT, 0))

    e, _, _, _, _, _ = make()
    e.initialize(mu[neg:neg + 1], -np.eye(man.D)[None], first=neg)
    mu_b, cov_b, _ = e.state()
    X, st = export(e)
    expect_x = np.zeros(n, dtype=np.uint32)
    expect_x[dead], expect_x[neg] = ST_UNINIT, ST_CHOLESKY
    assert np.array_equal(st, expect_x)
    XX = host(propagate(e, model, name, par[name], X))
    assert np.isnan(XX[neg]).all() and np.array_equal(np.delete(XX, [dead, neg], 0), np.delete(XXc, [dead, neg], 0))
    XX[dead] = XXc[0]
    XX[nan_s, 2 * man.D, man.S - 1] = np.nan   # the last scalar of the record
    Rb, act = R.copy(), np.ones(n, dtype=np.uint8)
    Rb[nan_r, man.D - 1, 0] = np.nan
    Rb[upper, 0, man.D - 1] = np.nan
    act[idle] = 0
    got = run(e, XX, Rb, active=act)
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[idle] = ST_UNINIT, ST_INACTIVE
    expect[[nan_s, nan_r, neg]] = ST_NONFINITE
    assert np.array_equal(got["status"], expect), (got["status"], expect)
    assert np.array_equal(e.status(), expect)
    e.close()
    failing = expect != 0
    assert np.array_equal(got["mu"][failing], mu_b[failing], equal_nan=True) and np.array_equal(got["cov"][failing], cov_b[failing], equal_nan=True)
    assert np.isnan(got["out_mu"][failing]).all() and np.isnan(got["out_cov"][failing]).all()
    assert same(got, clean, ALL_KEYS, rows=~failing)
    assert not np.array_equal(got["mu"][upper], mu[upper])
    ref = pr.predict_sampled(man, mu_b, cov_b, XX, Rb, active=act, initialised=init)
    assert np.array_equal(ref["status"], expect)


# ------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(spe):
    c = smc.case(spe, "pose", "f64", 255)
    e = smc.engine_of(spe, c)
    n, pts = c.n, 2 * e.D + 1
    lib = spe.load_library()
    buf = torch.zeros(n * pts * e.S, dtype=torch.float64, device="cuda")
    sent = torch.full((n * e.S,), -7.0, dtype=torch.float64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    out = spe.PredictSampledOut(sent.data_ptr(), None, st.data_ptr())
    good = spe.PredictSampledIn(p, p, 0, None)
    for args in ((None, p, 0), (p, None, 0), (p, p, 2), (p, p, -1)):   # code 1 = UKFB_ERR_INVALID_ARG
        pin = spe.PredictSampledIn(args[0], args[1], args[2], None)
        for commit in (0, 1):
            assert lib.ukfb_predict_sampled_dev(e._h, C.byref(pin), C.c_int(commit), C.byref(out)) == 1
    assert lib.ukfb_predict_sampled_dev(e._h, None, C.c_int(1), C.byref(out)) == 1
    assert lib.ukfb_predict_sampled_dev(e._h, C.byref(good), C.c_int(0), None) == 1
    assert lib.ukfb_predict_sampled_dev(e._h, C.byref(good), C.c_int(0), C.byref(spe.PredictSampledOut(None, None, None))) == 1
    assert lib.ukfb_predict_sampled_dev(e._h, C.byref(good), C.c_int(2), C.byref(out)) == 1
    assert lib.ukfb_predict_sampled_dev(e._h, C.byref(good), C.c_int(-1), C.byref(out)) == 1
    with pytest.raises(spe.UkfbError, match="code 1"):
        e.predict_sampled_dev(buf, buf, commit=False)
    torch.cuda.synchronize()
    assert np.array_equal(e.state()[0], c.mu) and np.array_equal(e.state()[1], c.cov) and (e.status() == 0).all()
    assert (buf == 0).all() and (sent == -7.0).all() and (st == -1).all()
    e.close()


# ---------------------------------------------------------------------------------------------- 8. host form on fp32 engines
@pytest.mark.parametrize("pname", ["f32", "f32w"])
def test_host_array_form_fp32(spe, pname):
    """fp32 engines: the host form narrows / widens the host doubles itself; its outputs and the committed state are the bits
    of the device form fed the same values rounded to float32.  Five filters."""
    n = 5
    c = smc.case(spe, "pose", pname, n)
    par, R = user(c)
    e, twin = smc.engine_of(spe, c), smc.engine_of(spe, c)
    X, _, st = e.sigma_points()
    assert (st == 0).all()
    rng = np.random.default_rng(9)
    XX = pr.user_f("pose", "drag", X, pr.expand(par["drag"])) + 1e-9 * rng.standard_normal(X.shape)   # NOT fp32 values
    Rh = R * (1.0 + 1e-9)
    assert not np.array_equal(XX, stored(XX, np.float32)) and not np.array_equal(Rh, stored(Rh, np.float32))
    o = e.predict_sampled(XX, Rh)
    mu_h, cov_h, _ = e.state()
    d = run(twin, stored(XX, np.float32), stored(Rh, np.float32))
    assert np.array_equal(o["mu"], d["out_mu"]) and np.array_equal(o["cov"], d["out_cov"]) and np.array_equal(o["status"], d["status"])
    assert np.array_equal(mu_h, d["mu"]) and np.array_equal(cov_h, d["cov"]) and np.array_equal(e.status(), twin.status())
    assert (o["status"] == 0).all() and not np.array_equal(mu_h, c.mu)
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------- 9. the two halves compose
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_predict_and_update_compose(spe, model):
    """three cycles of export -> user f -> predict_sampled_dev -> export -> user h (m = 3) -> update_sampled_dev against the same
    three cycles of the two references on the CPU, each fed the samples the device chain produced"""
    n, m = 64, 3
    c = smc.case(spe, model, "f64", n)
    man = man_of(model)
    par, R = user(c)
    b, r, noise, Q = sm.make_inputs(model, c.mu, c.dtype)
    z = sm.user_h(model, m, c.mu, b, r) + noise[m]
    name = pr.USER_MODELS[model][-1]
    e = smc.engine_of(spe, c)
    zd, qd = dev(e, z), dev(e, Q[m])
    mu_r, cov_r = c.mu.copy(), c.cov.copy()
    for cyc in range(3):
        X, st = export(e)
        assert (st == 0).all()
        XX = propagate(e, model, name, par[name], X).contiguous()
        p = run(e, XX, R)
        ref = pr.predict_sampled(man, mu_r, cov_r, host(XX), R)
        assert (p["status"] == 0).all() and (ref["status"] == 0).all()
        X, st = export(e)
        assert (st == 0).all()
        Z = sm.user_h(model, m, X, dev(e, b)[:, None, :], dev(e, r)[:, None, :]).contiguous()
        ust = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        e.update_sampled_dev(m, Z, zd, qd, status=ust)
        e.sync()
        torch.cuda.synchronize()
        upd = sm.update_sampled(man, ref["mu"], ref["cov"], host(Z), z, Q[m])
        assert (ust.cpu().numpy() == 0).all() and (upd["status"] == 0).all()
        mu_r, cov_r = upd["mu"], upd["cov"]
    mu_g, cov_g, _ = e.state()
    e.close()
    errs = (scaled(mu_g, mu_r), scaled(cov_g, cov_r))
    print(f"PARITY predict_sampled compose {model} n={n} cycles=3 dmu={errs[0]:.3e} dcov={errs[1]:.3e} tol={c.tol:.3e}")
    assert all(v <= c.tol for v in errs), errs
    assert not np.array_equal(mu_g, c.mu)


# --------------------------------------------------------------------------------------------------------- 10. graph capture
def test_recorded_in_a_graph(spe):
    """export -> f (torch) -> predict_sampled_dev recorded once in a torch.cuda.graph on the engine's stream (one branch) and
    replayed twice: the state of two direct rounds on a twin, bit for bit.  (The prediction alone does not read the state; with
    the export and f in front of it the second replay starts from what the first one committed.)"""
    n, model, name = 64, "pose", "drag"
    c = smc.case(spe, model, "f64", n)
    par, R = user(c)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()

    def make(stream):
        e = spe.BatchPoseUKF(n, precision=0, stream=stream)
        e.initialize(c.mu, c.cov)
        e.sync()
        return e

    def buffers(e):
        X = torch.zeros((n, 2 * e.D + 1, e.S), dtype=torch.float64, device="cuda")
        XX = torch.zeros_like(X)
        pt = {k: dev(e, v) for k, v in pr.expand(par[name]).items()}
        return X, XX, pt, dev(e, R)

    def round_(e, X, XX, pt, Rd):
        e.sigma_points_dev(X, None, None)
        XX.copy_(pr.user_f(model, name, X, pt))
        e.predict_sampled_dev(XX, Rd)

    twin = make(None)   # on torch's current stream: the export, f and the prediction are ordered by it
    tb = buffers(twin)
    for _ in range(2):
        round_(twin, *tb)
    twin.sync()
    torch.cuda.synchronize()
    mu_t, cov_t, _ = twin.state()
    st_t = twin.status()
    twin.close()

    eng = make(int(side.cuda_stream))
    assert eng.stream_kind == "given"
    gb = buffers(eng)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        round_(eng, *gb)
    torch.cuda.synchronize()
    assert np.array_equal(eng.state()[0], c.mu), "recording must not execute the call"
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    mu_g, cov_g, _ = eng.state()
    assert np.array_equal(mu_g, mu_t) and np.array_equal(cov_g, cov_t) and np.array_equal(eng.status(), st_t)
    assert (st_t == 0).all() and not np.array_equal(mu_g, c.mu)
    eng.close()
