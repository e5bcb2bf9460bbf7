"""Late samples on the device (ukfb_update_delayed_dev / ukfb_update_delayed / ukfb_delayed_lag_dev, include/ukf_batch.h).

The history is recorded with history_push_dev during real cycles on the HOT inputs of tests/delayed_reference.py (wide rotation
spreads, large rates and corrections: tests/test_delayed_reference.py shows that leaving out either transport of the chain moves
the result by 1e-3 ... 5e-2 scaled, far above every gate here) into a ring of 8 slots that the window of 6 steps wraps (first
slot 5).  The reference is tests/delayed_reference.py (pinned by tests/test_delayed_reference.py) run on the history and on the
engine's state AS DOWNLOADED.  Parity bound: |x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64) / 1e-4 (fp32) / 1e-9 + 2^-23 (fp32
engines with wide_arithmetic, against the reference's outputs rounded to fp32), and the scaled per-block comparison of
tests/feature_scaled_parity.py with that file's bounds (plain fp32: d_32 from delayed_reference.delayed_f32).  The maxima measured
on an MI355X are in profiles/delayed_parity.txt."""
import copy

import numpy as np
import pytest
import torch

import delayed_reference as dr
import feature_scaled_parity as fsp
import smoother_reference as sr
from engine_support import dev, host, new_engine, same_snapshot, scaled_ignoring_nan, snapshot, stored, tdt, unpack

pytestmark = pytest.mark.gpu

N = 1022   # not a multiple of four: the last workgroup holds two filters
STEPS, SLOTS, FIRST = 6, 8, 5
PRECS = [("f64", 0, 0, 1e-9), ("f32", 1, 0, 1e-4), ("f32w", 1, 1, 1e-9 + 2.0 ** -23)]
ACC_COV = 0.01 * np.eye(3)
ST_SKIPPED_SMALL_DT, ST_ERR_NEG_DT, ST_ERR_NONFINITE_MEAS, ST_ERR_CHOLESKY = 1 << 1, 1 << 2, 1 << 4, 1 << 5
ST_UNINITIALISED, ST_INACTIVE, ST_REJECTED_GATE = 1 << 7, 1 << 8, 1 << 9
UKFB_ERR_OUT_OF_RANGE = 4


def snap(e):
    """the engine's snapshot with the process noise of these filters"""
    return snapshot(e, range(min(e.capacity, 8)))


class Recording:
    """an engine at the window's last step, its history rings on the device, the inputs of every step"""


def record(spe, model, n, prec, wide, steps=STEPS, slots=SLOTS, first=FIRST, skip_init=(), per_filter_noise=False, inputs=None,
           late_at=None, late=None, **kw):
    """`steps` steps of real cycles on the hot inputs; inputs: replay a recording's inputs (they depend on the state they were
    drawn at); late = (models, z [n, 3], Q [3, 3]) is processed IN ORDER at step late_at through update_dev"""
    sy = spe.synth
    e = new_engine(spe, model, n, prec, wide, **kw)
    if per_filter_noise:
        scale = 1.0 + np.arange(n) / n + 0.5 * (np.arange(n) % 3 == 0)
        e.set_process_noise(scale[:, None, None] * e.process_noise()[None])
    mu0, cov0 = dr.hot_initial(sy, model, n)
    live = np.ones(n, bool)
    live[list(skip_init)] = False
    if skip_init:
        for i in np.nonzero(live)[0]:
            e.initialize(mu0[i:i + 1], cov0[i:i + 1], first=int(i))
    else:
        e.initialize(mu0, cov0)
    r = Recording()
    r.e, r.model, r.n, r.steps, r.slots, r.first, r.live, r.per_filter_noise = e, model, n, steps, slots, first, live, per_filter_noise
    r.mu_hist = torch.zeros((slots, n, e.S), dtype=tdt(e), device="cuda")
    r.cov_hist = torch.zeros((slots, n, e.PK), dtype=tdt(e), device="cuda")
    r.in_a = torch.zeros((slots, n, 3), dtype=tdt(e), device="cuda")
    r.in_b = torch.zeros((slots, n, 3), dtype=tdt(e), device="cuda")
    r.dt = np.array([dr.HOT_DT * (1.0 + 0.1 * (c % 7)) for c in range(steps - 1)])
    r.inputs = []
    for c in range(steps):
        slot = (first + c) % slots
        if inputs is None:
            mu_now = np.where(live[:, None], e.state(with_cov=False)[0], mu0)
            a, b, mid, z, Q = dr.hot_cycle_inputs(sy, model, n, c, mu_now)
        else:
            a, b, mid, z, Q = inputs[c]
        r.inputs.append((a, b, mid, z, Q))
        if c > 0:
            e.cycle(float(r.dt[c - 1]), int(mid), z, Q)
        if late_at == c:
            models, zl, Ql = late
            e.update_dev(0, dev(e, zl), dev(e, np.broadcast_to(Ql.reshape(1, 9), (n, 9))), meas_model_dev=dev(e, models, torch.int32))
        e.history_push_dev(slots, slot, r.mu_hist, r.cov_hist)
        if model == "pose":
            e.set_acceleration(a, ACC_COV)
        else:
            e.set_orient_inputs(b, a)
        r.in_a[slot] = dev(e, a)
        r.in_b[slot] = dev(e, b)
    r.latch_a, r.latch_b = a.astype(e.dtype).astype(np.float64), b.astype(e.dtype).astype(np.float64)
    return r


def params(spe, r):
    e, sy = r.e, spe.synth
    R = np.array([e.process_noise(i) for i in range(r.n)]) if r.per_filter_noise else e.process_noise()
    R = np.asarray(R, dtype=e.dtype).astype(np.float64)
    cfg = e.config()
    kw = dict(min_dt=cfg.min_time_delta, max_dt=cfg.max_time_delta)
    if r.model == "pose":
        return sr.Params("pose", R, acc_cov=np.asarray(2.0 * ACC_COV, dtype=e.dtype).astype(np.float64) / 2.0, **kw)
    from oracle import ukf_numpy as on
    return sr.Params("orient", R, tau_g=sy.ORIENT_TAU, tau_a=sy.ORIENT_TAU, earth=on.earth_rotation(sy.ORIENT_LATITUDE), **kw)


def reference(spe, r, lag, models, z, Q, dt=None, rings=True, mu_hist=None, cov_hist=None, gate_chi2=-1.0):
    """-> (result dict of delayed_reference.update_delayed, the call's arguments for the fp32 evaluation)"""
    e = r.e
    mu = sr.window_order((r.mu_hist if mu_hist is None else mu_hist).double().cpu().numpy(), r.first, r.steps)
    cov = sr.window_order(unpack(host(r.cov_hist if cov_hist is None else cov_hist), e.D), r.first, r.steps)
    a = sr.window_order(r.in_a.double().cpu().numpy(), r.first, r.steps)
    b = sr.window_order(r.in_b.double().cpu().numpy(), r.first, r.steps)
    if not rings:
        a, b = r.latch_a, r.latch_b
    if r.model == "pose":
        b = None
    mu_n, cov_n, _ = e.state()
    p = params(spe, r)
    dt = (r.dt if dt is None else dt)[:r.steps - 1]
    call = (p, mu, cov, mu_n, cov_n, dt, lag, models, stored(z, e.dtype), stored(Q, e.dtype))
    return dr.update_delayed(*call, in_a=a, in_b=b, initialised=r.live, gate_chi2=gate_chi2), call + (a, b)


def run(r, lag, models, z, Q, commit=False, dt=None, rings=True, mu_hist=None, cov_hist=None, outputs=True, e=None):
    """-> dict of NumPy arrays (float64; cov_out unpacked), and in ["raw"] the device tensors"""
    e = r.e if e is None else e
    n = r.n
    t = tdt(e)
    per = lambda x: x if np.isscalar(x) else dev(e, np.asarray(x, dtype=np.int32), torch.int32)   # noqa: E731
    Q = np.asarray(Q, dtype=np.float64)
    uniform_q = Q.size == 9
    o = {}
    if outputs:
        nan = lambda *s: torch.full(s, float("nan"), dtype=t, device="cuda")   # noqa: E731
        o = dict(z_pred=nan(n, 4), S=nan(n, 9), innov=nan(n, 3), maha=nan(n), loglik=nan(n), mu_out=nan(n, e.S), cov_out=nan(n, e.PK),
                 status=torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    e.update_delayed_dev((r.dt if dt is None else dt)[:r.steps - 1], r.slots, r.first, r.mu_hist if mu_hist is None else mu_hist,
                         r.cov_hist if cov_hist is None else cov_hist, per(lag), per(models), dev(e, z), dev(e, Q.reshape(-1, 9)),
                         q_is_uniform=uniform_q, in_a_dev=r.in_a if rings else None, in_b_dev=r.in_b if rings else None,
                         commit=commit, **o)
    torch.cuda.synchronize()
    out = {k: v.double().cpu().numpy() for k, v in o.items() if k not in ("status", "cov_out")}
    if outputs:
        out["status"] = o["status"].cpu().numpy().astype(np.uint32)
        out["cov_out"] = unpack(host(o["cov_out"]), e.D)
        out["S"] = out["S"].reshape(n, 3, 3)
    out["raw"] = o
    return out


def same_nan(x, ref):
    return np.array_equal(np.isnan(x), np.isnan(ref))


def check_parity(name, r, got, ref, call, tol, pname, rows=None):
    """mu_out / cov_out and the five statistics against the reference, then the scaled per-block comparison of the state"""
    res = ref
    rows = res["committed"] if rows is None else rows
    rnd = (lambda x: x.astype(np.float32).astype(np.float64)) if pname == "f32w" else (lambda x: x)
    assert np.array_equal(got["status"], res["status"]), (name, np.unique(got["status"]), np.unique(res["status"]))
    figs = {}
    for k in ("mu_out", "cov_out", "z_pred", "S", "innov", "maha", "loglik"):
        assert same_nan(got[k], res[k]), (name, k)
        figs[k] = scaled_ignoring_nan(got[k], rnd(res[k]))
    print(f"PARITY delayed/{name} n={r.n} " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()) + f" tol={tol:.3e}")
    for k, v in figs.items():
        assert v <= tol, (name, k, v, tol)
    if rows.any():
        p, mu, cov, mu_n, cov_n, dt, lag, models, z, Q, a, b = call

        def f32():
            i = np.nonzero(rows)[0]
            q = copy.copy(p)
            if np.ndim(q.R) == 3:
                q.R = q.R[i]
            lg = np.broadcast_to(lag, (r.n,))[i]
            md = np.broadcast_to(models, (r.n,))[i]
            QQ = np.broadcast_to(Q, (r.n, 3, 3))[i]
            aa = None if a is None else (a[:, i] if np.ndim(a) == 3 else a[i])
            bb = None if b is None else (b[:, i] if np.ndim(b) == 3 else b[i])
            return tuple(dr.delayed_f32(q, mu[:, i], cov[:, i], mu_n[i], cov_n[i], dt, lg, md, z[i], QQ, aa, bb, prec=pr)
                         for pr in ("f32", "f64"))
        fsp.judge_state("delayed/" + name, r.model, pname, got["mu_out"][rows], got["cov_out"][rows], res["mu_out"][rows],
                        res["cov_out"][rows], f32=f32)
    return figs


def sample(spe, r, lag):
    """the late sample of every filter, taken near the recorded state of its own step"""
    lag = np.broadcast_to(np.asarray(lag), (r.n,))
    s = np.clip(r.steps - 1 - lag, 0, r.steps - 1)
    mu = sr.window_order(r.mu_hist.double().cpu().numpy(), r.first, r.steps)
    mu_at = np.where(r.live[:, None], mu[s, np.arange(r.n)], dr.hot_initial(spe.synth, r.model, r.n)[0])
    return dr.hot_late_sample(spe.synth, r.model, r.n, mu_at)


_CACHE = {}


def recorded(spe, model, pname):
    key = (model, pname)
    if key not in _CACHE:
        _, prec, wide, _ = [p for p in PRECS if p[0] == pname][0]
        _CACHE[key] = record(spe, model, N, prec, wide)
    return _CACHE[key]


MIXED = np.arange(N) % STEPS   # lags 0 ... 5: the four rows of a wavefront differ


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_parity_commit_modes_and_outputs(spe, model, pname, prec, wide, tol):
    """mixed lags and (Pose) all nine models; commit = 0 keeps every bit of the engine; commit = 1 with out = NULL stores
    commit = 0's mu_out / cov_out bit for bit.  Runs on a fresh recording: it commits."""
    r = record(spe, model, N, prec, wide)
    r.e.set_last_measurement_time(np.arange(1, N + 1, dtype=np.int64) * 1000 + 7)
    models, z, Q = sample(spe, r, MIXED)
    ref, call = reference(spe, r, MIXED, models, z, Q)
    assert (ref["status"] == 0).all() and ref["committed"].all()
    before = snap(r.e)
    got = run(r, MIXED, models, z, Q, commit=False)
    assert same_snapshot(before, snap(r.e)), "commit = 0 changed the engine"
    check_parity(f"{model}/{pname}", r, got, ref, call, tol, pname)
    run(r, MIXED, models, z, Q, commit=True, outputs=False)
    after = snap(r.e)
    assert np.array_equal(after[0], got["mu_out"]) and np.array_equal(after[1], got["cov_out"])
    assert (after[3] == 0).all() and all(np.array_equal(x, y) for x, y in zip(before[4:6], after[4:6]))   # times and noise stay
    r.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_uniform_lag_is_the_lag_array_bit_for_bit(spe, model):
    r = recorded(spe, model, "f64")
    models, z, Q = sample(spe, r, 3)
    a = run(r, 3, models, z, Q)
    b = run(r, np.full(N, 3), models, z, Q)
    assert (a["status"] == 0).all()
    for k in ("mu_out", "cov_out", "z_pred", "S", "innov", "maha", "loglik", "status"):
        assert np.array_equal(a[k], b[k]), k
    ref, call = reference(spe, r, 3, models, z, Q)
    check_parity(f"{model}/f64/uniform-lag-3", r, a, ref, call, 1e-9, "f64")


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_lag_zero_is_the_ordinary_update(spe, model, pname, prec, wide, tol):
    """against ukfb_update_dev on a twin engine, within the parity tolerance (the update kernel uses closed forms for the
    selections: no bit identity)"""
    r = record(spe, model, 254, prec, wide)
    twin = record(spe, model, 254, prec, wide)
    models, z, Q = sample(spe, r, 0)
    got = run(r, 0, models, z, Q)
    e = twin.e
    e.update_dev(0, dev(e, z), dev(e, np.broadcast_to(Q.reshape(1, 9), (254, 9))), meas_model_dev=dev(e, models, torch.int32))
    mu_t, cov_t, _ = e.state()
    assert (got["status"] == 0).all() and (e.status() == 0).all()
    em, ec = scaled_ignoring_nan(got["mu_out"], mu_t), scaled_ignoring_nan(got["cov_out"], cov_t)
    print(f"PARITY delayed/{model}/{pname}/lag-0 against update_dev: mu {em:.3e} cov {ec:.3e} tol={tol:.3e}")
    assert em <= tol and ec <= tol
    r.e.close(); twin.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_filters_that_commit_nothing_keep_every_bit(spe, model):
    n = 64
    dead = 22
    r = record(spe, model, n, 0, 0, skip_init=(dead,))
    lag = np.arange(n) % STEPS
    models, z, Q = sample(spe, r, lag)
    clean = run(r, lag, models, z, Q)
    lag2, models2, z2 = lag.copy(), models.copy(), z.copy()
    lag2[1], lag2[2], lag2[3] = STEPS, 1000, -1
    models2[5] = -1
    models2[6] = 9 if model == "pose" else 0
    z2[9, 0] = np.nan
    z2[10, 2] = np.inf
    if model == "pose":
        models2[10] = 0
    # poisoned history records inside the chains of filters 13 (a non-positive covariance) and 14 (a NaN in the mean); filter 15
    # has the same poison BELOW its chain and stays healthy
    lag2[13], lag2[14], lag2[15] = 3, 4, 1
    for i in (13, 14, 15):
        models2[i], z2[i] = models[i], z[i]
    ch, mh = r.cov_hist.clone(), r.mu_hist.clone()
    D = r.e.D
    ind = torch.from_numpy(-np.eye(D)[np.tril_indices(D)]).to("cuda", ch.dtype)
    ch[(FIRST + 3) % SLOTS, 13] = ind
    mh[(FIRST + 2) % SLOTS, 14, 1] = float("nan")
    ch[(FIRST + 1) % SLOTS, 15] = ind
    ref, _ = reference(spe, r, lag2, models2, z2, Q, mu_hist=mh, cov_hist=ch)
    before = snap(r.e)
    got = run(r, lag2, models2, z2, Q, mu_hist=mh, cov_hist=ch)
    st = got["status"]
    assert np.array_equal(st, ref["status"]), (st, ref["status"])
    assert st[1] == ST_ERR_NEG_DT and st[2] == ST_ERR_NEG_DT and st[3] == ST_INACTIVE and st[5] == ST_INACTIVE and st[6] == ST_INACTIVE
    assert st[9] == ST_ERR_NONFINITE_MEAS and st[10] == ST_ERR_NONFINITE_MEAS and st[dead] == ST_UNINITIALISED
    assert st[13] == ST_ERR_CHOLESKY and st[14] == ST_ERR_CHOLESKY and st[15] == 0
    quiet = np.array([1, 2, 3, 5, 6, 9, 10, 13, 14, dead])
    for k in ("mu_out", "cov_out", "z_pred", "S", "innov", "maha", "loglik"):
        assert np.isnan(got[k][quiet]).all(), k
    # wave-mates (and filter 15): the bits of the run in which everybody is healthy -- their own lag, model and sample are unchanged
    same = np.ones(n, bool)
    same[quiet] = False
    same[15] = False
    for k in ("mu_out", "cov_out", "z_pred", "S", "innov", "maha", "loglik", "status"):
        assert np.array_equal(got[k][same], clean[k][same]), k
    assert scaled_ignoring_nan(got["mu_out"][15], ref["mu_out"][15]) <= 1e-9
    # committing: the quiet filters keep every bit of the engine, the others store mu_out
    run(r, lag2, models2, z2, Q, mu_hist=mh, cov_hist=ch, commit=True, outputs=False)
    after = snap(r.e)
    assert np.array_equal(after[0][quiet], before[0][quiet], equal_nan=True) and np.array_equal(after[1][quiet], before[1][quiet], equal_nan=True)
    keep = np.ones(n, bool)
    keep[quiet] = False
    assert np.array_equal(after[0][keep], got["mu_out"][keep]) and np.array_equal(after[1][keep], got["cov_out"][keep])
    assert np.array_equal(after[3], st), "commit = 1 writes the call's status to the engine's array"
    r.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_gate_rejects_with_outputs_written(spe, model):
    n = 64
    r = record(spe, model, n, 0, 0, gate_chi2=9.0)
    models, z, Q = sample(spe, r, 2)
    z = z.copy()
    z[::2] += 50.0 if model == "orient" else np.where(models[::2, None] == 3, 1.5, 50.0)
    ref, _ = reference(spe, r, 2, models, z, Q, gate_chi2=9.0)
    before = snap(r.e)
    got = run(r, 2, models, z, Q, commit=True)
    assert np.array_equal(got["status"], ref["status"])
    rej = got["status"] == ST_REJECTED_GATE
    assert rej[::2].all() and (got["status"][~rej] == 0).all() and (~rej).sum() >= n // 4   # (a few of the others are 3 sigma off too)
    assert np.isnan(got["mu_out"][rej]).all() and np.isfinite(got["maha"]).all() and np.isfinite(got["S"]).all()
    for k in ("z_pred", "S", "innov", "maha", "loglik"):
        assert scaled_ignoring_nan(got[k], ref[k]) <= 1e-9, k
    after = snap(r.e)
    assert np.array_equal(after[0][rej], before[0][rej]) and np.array_equal(after[1][rej], before[1][rej])
    assert np.array_equal(after[0][~rej], got["mu_out"][~rej]) and np.array_equal(after[3], got["status"])
    r.e.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS[:2], ids=[p[0] for p in PRECS[:2]])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_window_edge_cases(spe, model, pname, prec, wide, tol):
    """a gated dt in the middle of the window, per-filter process noise, ring inputs against latched inputs"""
    n = 254
    r = record(spe, model, n, prec, wide, per_filter_noise=True)
    lag = np.arange(n) % STEPS
    models, z, Q = sample(spe, r, lag)
    outs = {}
    for rings in (True, False):
        ref, call = reference(spe, r, lag, models, z, Q, rings=rings)
        outs[rings] = run(r, lag, models, z, Q, rings=rings)
        check_parity(f"{model}/{pname}/per-filter-noise/{'rings' if rings else 'latches'}", r, outs[rings], ref, call, tol, pname)
    assert not np.array_equal(outs[True]["mu_out"], outs[False]["mu_out"])
    dt = r.dt.copy()
    dt[2] = 0.0   # the prediction 2 -> 3: inside the chains of lags 3, 4, 5
    ref, call = reference(spe, r, lag, models, z, Q, dt=dt)
    got = run(r, lag, models, z, Q, dt=dt)
    assert (got["status"][lag >= 3] == ST_SKIPPED_SMALL_DT).all() and (got["status"][lag < 3] == 0).all()
    check_parity(f"{model}/{pname}/gated-dt", r, got, ref, call, tol, pname)
    r.e.close()


def test_largest_window_and_one_step_more(spe):
    """33 steps with lag 32 on 130 filters (a ring of 40 that the window wraps); 34 steps: OUT_OF_RANGE, nothing written"""
    steps, slots, first, n = 33, 40, 20, 130
    r = record(spe, "pose", n, 0, 0, steps=steps, slots=slots, first=first)
    lag = np.where(np.arange(n) % 4 == 3, 17, 32)
    models, z, Q = sample(spe, r, lag)
    ref, call = reference(spe, r, lag, models, z, Q)
    got = run(r, lag, models, z, Q)
    check_parity("pose/f64/33-steps", r, got, ref, call, 1e-9, "f64")
    before = snap(r.e)
    out = torch.full((n, r.e.S), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(spe.engine.UkfbError) as err:
        r.e.update_delayed_dev(np.full(33, 0.05), slots, first, r.mu_hist, r.cov_hist, 32, 0, dev(r.e, z), dev(r.e, Q.reshape(1, 9)),
                               q_is_uniform=True, commit=True, mu_out=out, status=st)
    assert f"code {UKFB_ERR_OUT_OF_RANGE}" in str(err.value), str(err.value)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (st == -1).all() and same_snapshot(before, snap(r.e))
    r.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_end_to_end_late_against_in_order(spe, model, pname, prec, wide, tol):
    """engine A receives the sample in order (and the same later cycles), engine B late through this call:
    |B - A| <= |ref_B - ref_A| + tol (1 + |ref|) per component -- the reference's own gap plus the parity tolerance"""
    n, lag = 254, 3
    rb = record(spe, model, n, prec, wide)
    late = sample(spe, rb, lag)
    ra = record(spe, model, n, prec, wide, inputs=rb.inputs, late_at=STEPS - 1 - lag, late=late)
    models, z, Q = late
    ref_b, _ = reference(spe, rb, lag, models, z, Q)
    run(rb, lag, models, z, Q, commit=True, outputs=False)
    mu_a, cov_a, _ = ra.e.state()
    mu_b, cov_b, _ = rb.e.state()
    assert (rb.e.status() == 0).all() and ref_b["committed"].all()
    # ref_A: the same in-order processing by the NumPy oracle on the same inputs
    from oracle import ukf_numpy as on
    mu_ra, cov_ra = in_order_reference(spe, on, model, rb, late, STEPS - 1 - lag)
    # (both references as the engines store them: the wide mode's tolerance is two roundings of the storage format)
    rnd = (lambda x: x.astype(np.float32).astype(np.float64)) if pname == "f32w" else (lambda x: x)
    gap_mu, gap_cov = np.abs(rnd(ref_b["mu"]) - mu_ra), np.abs(rnd(ref_b["cov"]) - cov_ra)
    over_mu = np.abs(mu_b - mu_a) - gap_mu - tol * (1.0 + np.abs(mu_ra))
    over_cov = np.abs(cov_b - cov_a) - gap_cov - tol * (1.0 + np.abs(cov_ra))
    print(f"END-TO-END delayed/{model}/{pname}: max |B - A| mu {np.abs(mu_b - mu_a).max():.3e} cov {np.abs(cov_b - cov_a).max():.3e}; "
          f"reference gap mu {gap_mu.max():.3e} cov {gap_cov.max():.3e}; largest excess over the bound mu {over_mu.max():.3e} "
          f"cov {over_cov.max():.3e}")
    assert (over_mu <= 0).all() and (over_cov <= 0).all()
    ra.e.close(); rb.e.close()


def in_order_reference(spe, on, model, rb, late, late_at):
    """Engine A by the NumPy oracle: from the recording's DOWNLOADED record of step late_at (engine A held the same bits there
    before the late sample) the sample in order, then the recorded cycles up to the present, on the inputs and parameters as
    the engine stores them, the state rounded to the engine's storage after every call as the engine rounds it"""
    e, n = rb.e, rb.n
    p = params(spe, rb)
    rnd = lambda x: stored(x, e.dtype)   # noqa: E731
    mu = sr.window_order(rb.mu_hist.double().cpu().numpy(), rb.first, rb.steps)[late_at]
    cov = sr.window_order(unpack(host(rb.cov_hist), e.D), rb.first, rb.steps)[late_at]
    models, zl, Ql = late
    QQ = rnd(np.broadcast_to(Ql, (n, 3, 3)))
    mu, cov, st = on.pose_update_mixed(mu, cov, models, rnd(zl), QQ) if model == "pose" else on.orient_update(mu, cov, rnd(zl), QQ)
    assert not st.any()
    mu, cov = rnd(mu), rnd(cov)
    for c in range(late_at + 1, rb.steps):
        a, b = rnd(rb.inputs[c - 1][0]), rnd(rb.inputs[c - 1][1])
        _, _, mid, z, Q = rb.inputs[c]
        if model == "pose":
            mu, cov, s1 = on.pose_predict(mu, cov, p.R, a, p.acc_cov, rb.dt[c - 1])
            mu, cov, s2 = on.pose_update(mu, cov, mid, rnd(z), rnd(Q))
        else:
            mu, cov, s1 = on.orient_predict(mu, cov, p.R, a, b, p.tau_g, p.tau_a, p.earth, rb.dt[c - 1])
            mu, cov, s2 = on.orient_update(mu, cov, rnd(z), rnd(Q))
        assert not s1.any() and not s2.any()
        mu, cov = rnd(mu), rnd(cov)
    return mu, cov


def test_delayed_lag_dev_against_the_host_rule(spe):
    n = 1022
    e = spe.BatchPoseUKF(n, precision=spe.F32)
    ts = np.array([1000, 2000, 3100, 4000, 5000, 6500], dtype=np.int64)
    rng = np.random.default_rng(3)
    t = rng.integers(-2000, 9000, n).astype(np.int64)
    t[:16] = [6500, 9000, 6499, 5750, 5751, 5749, 3550, 1000, 600, 500, 499, -7000, 2550, 1500, 4500, 2**40]
    td = torch.from_numpy(t).cuda()
    out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    e.delayed_lag_dev(ts, td, out)
    torch.cuda.synchronize()
    want = dr.lag_rule(ts, t)
    assert np.array_equal(out.cpu().numpy(), want)
    assert list(want[:14]) == [0, 0, 0, 1, 0, 1, 3, 5, 5, 5, 6, 6, 4, 5]
    # one step: every sample not newer than it is out of the window unless it is the step's own stamp ... or nearer than nothing
    e.delayed_lag_dev(ts[:1], td, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), dr.lag_rule(ts[:1], t))
    e.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_host_array_form(spe, pname, prec, wide, tol):
    r = recorded(spe, "pose", pname)
    models, z, Q = sample(spe, r, MIXED)
    devf = run(r, MIXED, models, z, Q)
    mu = sr.window_order(r.mu_hist.double().cpu().numpy(), FIRST, STEPS)
    cov = sr.window_order(unpack(host(r.cov_hist), r.e.D), FIRST, STEPS)
    a = sr.window_order(r.in_a.double().cpu().numpy(), FIRST, STEPS)
    o = r.e.update_delayed(r.dt, mu, cov, MIXED, models, z, np.broadcast_to(Q, (N, 3, 3)), in_a=a, commit=False)
    assert (o["status"] == 0).all()
    for k in ("mu_out", "cov_out", "z_pred", "S", "innov", "maha", "loglik"):
        assert np.array_equal(o[k], devf[k]), k   # the same records in, the same kernel
