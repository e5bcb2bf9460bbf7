"""Relative measurements on the device (ukfb_update_relative_dev / ukfb_update_relative, include/ukf_batch_relative.h).

The history is recorded with history_push_dev during real cycles on the HOT inputs of tests/delayed_reference.py
(tests/relative_cases.record) into a ring of 8 slots that the window of 6 steps wraps (first slot 5).  The reference is
tests/relative_reference.py (pinned by tests/test_relative_reference.py) run on the history and on the engine's state AS
DOWNLOADED.  Parity bound, as tests/test_gpu_delayed.py: |x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64) / 1e-4 (fp32) /
1e-9 + 2^-23 (fp32 engines with wide_arithmetic, against the reference's outputs rounded to fp32), and the scaled per-block
comparison of tests/feature_scaled_parity.py with that file's bounds (plain fp32: d_32 from relative_reference.relative_f32).
The maxima measured on an MI355X are in profiles/relative_parity.txt."""
import numpy as np
import pytest
import torch

import feature_scaled_parity as fsp
import relative_cases as rc
import relative_reference as rr
import smoother_reference as sr
from engine_support import dev, host, new_engine, same_snapshot, scaled_ignoring_nan, snapshot, stored, tdt, unpack

pytestmark = pytest.mark.gpu

N = 254   # not a multiple of four: the last workgroup holds two filters
STEPS, SLOTS, FIRST = 6, 8, 5
PRECS = [("f64", 0, 0, 1e-9), ("f32", 1, 0, 1e-4), ("f32w", 1, 1, 1e-9 + 2.0 ** -23)]
ST_ERR_NEG_DT, ST_ERR_NONFINITE_MEAS, ST_ERR_CHOLESKY = 1 << 2, 1 << 4, 1 << 5
ST_UNINITIALISED, ST_INACTIVE, ST_REJECTED_GATE = 1 << 7, 1 << 8, 1 << 9
UKFB_ERR_OUT_OF_RANGE, UKFB_ERR_WRONG_MODEL = 4, 5
FLOATS = ("mu_out", "cov_out", "z_pred", "S", "innov", "maha", "loglik")


def snap(e):
    return snapshot(e, range(min(e.capacity, 8)))


def window(r, mu_hist=None, cov_hist=None):
    """the ring as downloaded, in window order -> (mu, cov, in_a)"""
    e = r.e
    mu = sr.window_order((r.mu_hist if mu_hist is None else mu_hist).double().cpu().numpy(), r.first, r.steps)
    cov = sr.window_order(unpack(host(r.cov_hist if cov_hist is None else cov_hist), e.D), r.first, r.steps)
    return mu, cov, sr.window_order(r.in_a.double().cpu().numpy(), r.first, r.steps)


def reference(r, lag, models, z, Q, mu_hist=None, cov_hist=None, gate_chi2=-1.0):
    """-> (result dict of relative_reference.update_relative, the call's arguments for the fp32 evaluation)"""
    e = r.e
    mu, cov, a = window(r, mu_hist, cov_hist)
    mu_n, cov_n, _ = e.state()
    call = (rc.params(r), mu, cov, mu_n, cov_n, r.dt[:r.steps - 1], lag, models, stored(z, e.dtype), stored(Q, e.dtype))
    return rr.update_relative(*call, in_a=a, initialised=r.live, gate_chi2=gate_chi2), call + (a,)


def run(r, lag, models, z, Q, commit=False, mu_hist=None, cov_hist=None, outputs=True):
    """-> dict of NumPy arrays (float64; cov_out unpacked, S [n, 6, 6]), and in ["raw"] the device tensors"""
    e, n = r.e, r.n
    t = tdt(e)
    per = lambda x: int(x) if np.isscalar(x) else dev(e, np.asarray(x, dtype=np.int32), torch.int32)   # noqa: E731
    Q = np.asarray(Q, dtype=np.float64)
    o = {}
    if outputs:
        nan = lambda *s: torch.full(s, float("nan"), dtype=t, device="cuda")   # noqa: E731
        o = dict(z_pred=nan(n, 7), S=nan(n, 36), innov=nan(n, 6), maha=nan(n), loglik=nan(n), mu_out=nan(n, e.S), cov_out=nan(n, e.PK),
                 status=torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    e.update_relative_dev(r.dt[:r.steps - 1], r.slots, r.first, r.mu_hist if mu_hist is None else mu_hist,
                          r.cov_hist if cov_hist is None else cov_hist, per(lag), per(models), dev(e, z), dev(e, Q.reshape(-1, 36)),
                          q_is_uniform=Q.size == 36, in_a_dev=r.in_a, commit=commit, **o)
    torch.cuda.synchronize()
    out = {k: v.double().cpu().numpy() for k, v in o.items() if k not in ("status", "cov_out")}
    if outputs:
        out["status"] = o["status"].cpu().numpy().astype(np.uint32)
        out["cov_out"] = unpack(host(o["cov_out"]), e.D)
        out["S"] = out["S"].reshape(n, 6, 6)
    out["raw"] = o
    return out


def check_parity(name, r, got, ref, call, tol, pname):
    """mu_out / cov_out and the five scores against the reference, then the scaled per-block comparison of the state"""
    rows = ref["committed"]
    rnd = (lambda x: x.astype(np.float32).astype(np.float64)) if pname == "f32w" else (lambda x: x)
    assert np.array_equal(got["status"], ref["status"]), (name, np.unique(got["status"]), np.unique(ref["status"]))
    figs = {}
    for k in FLOATS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
        figs[k] = scaled_ignoring_nan(got[k], rnd(ref[k]))
    print(f"PARITY relative/{name} n={r.n} " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()) + f" tol={tol:.3e}")
    for k, v in figs.items():
        assert v <= tol, (name, k, v, tol)
    if rows.any():
        p, mu, cov, mu_n, cov_n, dt, lag, models, z, Q, a = call

        def f32():
            i = np.nonzero(rows)[0]
            lg, md = np.broadcast_to(lag, (r.n,))[i], np.broadcast_to(models, (r.n,))[i]
            zz = np.where(np.isnan(z[i]), 0.0, z[i])   # (the part a model does not read)
            QQ = np.broadcast_to(Q, (r.n, 6, 6))[i]
            return tuple(rr.relative_f32(p, mu[:, i], cov[:, i], mu_n[i], cov_n[i], dt, lg, md, zz, QQ, a[:, i], prec=pr)
                         for pr in ("f32", "f64"))
        fsp.judge_state("relative/" + name, "pose", pname, got["mu_out"][rows], got["cov_out"][rows], ref["mu_out"][rows],
                        ref["cov_out"][rows], f32=f32)
    return figs


def sample(spe, r, lag):
    """the increment of every filter, taken between the recorded state of its own step and the present"""
    lag = np.broadcast_to(np.asarray(lag), (r.n,))
    s = np.clip(r.steps - 1 - lag, 0, r.steps - 1)
    mu = sr.window_order(r.mu_hist.double().cpu().numpy(), r.first, r.steps)
    mu0 = rc.dr.hot_initial(spe.synth, "pose", r.n)[0]
    mu_s = np.where(r.live[:, None], mu[s, np.arange(r.n)], mu0)
    mu_n = np.where(r.live[:, None], r.e.state(with_cov=False)[0], mu0)
    return rc.increments(spe, r.n, mu_n, mu_s)


def record(spe, n, prec, wide, **kw):
    return rc.record(spe, n, prec, wide, kw.pop("steps", STEPS), kw.pop("slots", SLOTS), kw.pop("first", FIRST), **kw)


_CACHE = {}


def recorded(spe, pname):
    """one recording per precision, shared by the tests that commit nothing"""
    if pname not in _CACHE:
        _, prec, wide, _ = [p for p in PRECS if p[0] == pname][0]
        _CACHE[pname] = record(spe, N, prec, wide)
    return _CACHE[pname]


MIXED = 1 + np.arange(N) % 5   # lags 1 ... 5: the four rows of a wavefront differ


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_parity_commit_modes_and_outputs(spe, pname, prec, wide, tol):
    """mixed lags and models; commit = 0 keeps every bit of the engine; commit = 1 with out = NULL stores commit = 0's mu_out /
    cov_out bit for bit.  Runs on a fresh recording: it commits."""
    r = record(spe, N, prec, wide)
    r.e.set_last_measurement_time(np.arange(1, N + 1, dtype=np.int64) * 1000 + 7)
    models, z, Q = sample(spe, r, MIXED)
    ref, call = reference(r, MIXED, models, z, Q)
    assert (ref["status"] == 0).all() and ref["committed"].all() and not ref["clamped"].any()
    before = snap(r.e)
    got = run(r, MIXED, models, z, Q, commit=False)
    assert same_snapshot(before, snap(r.e)), "commit = 0 changed the engine"
    check_parity(pname, r, got, ref, call, tol, pname)
    # entries outside the model's part are zero
    m1, m2 = models == rr.POSITION, models == rr.ROTATION
    assert not got["z_pred"][m1, 3:].any() and not got["innov"][m1, 3:].any() and not got["S"][m1, 3:, :].any() and not got["S"][m1, :, 3:].any()
    assert not got["z_pred"][m2, :3].any() and not got["innov"][m2, :3].any() and not got["S"][m2, :3, :].any() and not got["S"][m2, :, :3].any()
    run(r, MIXED, models, z, Q, commit=True, outputs=False)
    after = snap(r.e)
    assert np.array_equal(after[0], got["mu_out"]) and np.array_equal(after[1], got["cov_out"])
    assert (after[3] == 0).all() and all(np.array_equal(x, y) for x, y in zip(before[4:6], after[4:6]))   # times and noise stay
    r.e.close()


def test_uniform_lag_and_model_are_the_arrays_bit_for_bit(spe):
    r = recorded(spe, "f64")
    _, z, Q = sample(spe, r, 3)
    z = np.where(np.isnan(z), 0.25, z)   # (every part finite: the model is uniform below)
    for model in (rr.POSE, rr.POSITION, rr.ROTATION):
        a = run(r, 3, model, z, Q)
        b = run(r, np.full(N, 3), np.full(N, model), z, np.broadcast_to(Q, (N, 6, 6)))
        assert (a["status"] == 0).all()
        for k in FLOATS + ("status",):
            assert np.array_equal(a[k], b[k]), (model, k)
    ref, call = reference(r, 3, rr.ROTATION, z, Q)
    check_parity("f64/uniform-lag-3-rotation", r, a, ref, call, 1e-9, "f64")


def test_filters_that_commit_nothing_keep_every_bit(spe):
    n = 64
    dead = 22
    r = record(spe, n, 0, 0, skip_init=(dead,))
    lag = 1 + np.arange(n) % 5
    models, z, Q = sample(spe, r, lag)
    QQ = np.broadcast_to(Q, (n, 6, 6)).copy()
    clean = run(r, lag, models, z, QQ)
    lag2, models2, z2, Q2 = lag.copy(), models.copy(), z.copy(), QQ.copy()
    lag2[1], lag2[2], lag2[3], lag2[4] = STEPS, 1000, -1, 0
    models2[5], models2[6] = -1, 3
    z2[9, 0] = np.nan                    # model 0 reads it
    z2[10, 4] = np.inf                   # model 1 does not: the filter stays healthy
    Q2[11, 5, 3] = np.nan                # model 2 reads the lower triangle of its rows and columns
    Q2[12, 0, 1] = np.nan                # the upper triangle is not read
    assert models[9] == rr.POSE and models[10] == rr.POSITION and models[11] == rr.ROTATION and models[12] == rr.POSE
    # poisoned history records inside the chains of filters 13 (a non-positive covariance) and 14 (a NaN in the mean); filter 15
    # has the same poison BELOW its chain and stays healthy
    lag2[13], lag2[14], lag2[15] = 3, 4, 1
    ch, mh = r.cov_hist.clone(), r.mu_hist.clone()
    D = r.e.D
    ind = torch.from_numpy(-np.eye(D)[np.tril_indices(D)]).to("cuda", ch.dtype)
    ch[(FIRST + 3) % SLOTS, 13] = ind
    mh[(FIRST + 2) % SLOTS, 14, 1] = float("nan")
    ch[(FIRST + 1) % SLOTS, 15] = ind
    ref, _ = reference(r, lag2, models2, z2, Q2, mu_hist=mh, cov_hist=ch)
    before = snap(r.e)
    got = run(r, lag2, models2, z2, Q2, mu_hist=mh, cov_hist=ch)
    st = got["status"]
    assert np.array_equal(st, ref["status"]), (st, ref["status"])
    assert st[1] == ST_ERR_NEG_DT and st[2] == ST_ERR_NEG_DT
    assert st[3] == ST_INACTIVE and st[4] == ST_INACTIVE and st[5] == ST_INACTIVE and st[6] == ST_INACTIVE
    assert st[9] == ST_ERR_NONFINITE_MEAS and st[11] == ST_ERR_NONFINITE_MEAS and st[10] == 0 and st[12] == 0
    assert st[dead] == ST_UNINITIALISED
    assert st[13] == ST_ERR_CHOLESKY and st[14] == ST_ERR_CHOLESKY and st[15] == 0
    quiet = np.array([1, 2, 3, 4, 5, 6, 9, 11, 13, 14, dead])
    for k in FLOATS:
        assert np.isnan(got[k][quiet]).all(), k
    # wave-mates: the bits of the run in which everybody is healthy -- their own lag, model and sample are unchanged
    same = np.ones(n, bool)
    same[quiet] = False
    same[[13, 14, 15]] = False
    for k in FLOATS + ("status",):
        assert np.array_equal(got[k][same], clean[k][same]), k
    assert scaled_ignoring_nan(got["mu_out"][15], ref["mu_out"][15]) <= 1e-9
    # committing: the quiet filters keep every bit of the engine, the others store mu_out
    run(r, lag2, models2, z2, Q2, mu_hist=mh, cov_hist=ch, commit=True, outputs=False)
    after = snap(r.e)
    assert np.array_equal(after[0][quiet], before[0][quiet], equal_nan=True) and np.array_equal(after[1][quiet], before[1][quiet], equal_nan=True)
    keep = np.ones(n, bool)
    keep[quiet] = False
    assert np.array_equal(after[0][keep], got["mu_out"][keep]) and np.array_equal(after[1][keep], got["cov_out"][keep])
    assert np.array_equal(after[3], st), "commit = 1 writes the call's status to the engine's array"
    r.e.close()


def test_gate_rejects_with_the_scores_written(spe):
    n = 64
    r = record(spe, n, 0, 0, gate_chi2=16.0)
    models, z, Q = sample(spe, r, 2)
    z = z.copy()
    z[::2, :3] += 50.0
    z[::2, 3:7] = rr.on.quat_mul(z[::2, 3:7], rr.on.so3_exp(np.full((n // 2, 3), 1.0), 1.0))
    ref, _ = reference(r, 2, models, z, Q, gate_chi2=16.0)
    before = snap(r.e)
    got = run(r, 2, models, z, Q, commit=True)
    assert np.array_equal(got["status"], ref["status"])
    rej = got["status"] == ST_REJECTED_GATE
    assert rej[::2].all() and (got["status"][~rej] == 0).all() and (~rej).sum() >= n // 4
    assert np.isnan(got["mu_out"][rej]).all() and np.isfinite(got["maha"]).all() and np.isfinite(got["S"]).all()
    for k in ("z_pred", "S", "innov", "maha", "loglik"):
        assert scaled_ignoring_nan(got[k], ref[k]) <= 1e-9, k
    after = snap(r.e)
    assert np.array_equal(after[0][rej], before[0][rej]) and np.array_equal(after[1][rej], before[1][rej])
    assert np.array_equal(after[0][~rej], got["mu_out"][~rej]) and np.array_equal(after[3], got["status"])
    r.e.close()


def test_largest_window_and_one_step_more(spe):
    """33 steps with lag 32 on 130 filters (a ring of 40 that the window wraps); 34 steps: OUT_OF_RANGE, nothing written"""
    steps, slots, first, n = 33, 40, 20, 130
    r = record(spe, n, 0, 0, steps=steps, slots=slots, first=first)
    lag = np.where(np.arange(n) % 4 == 3, 17, 32)
    models, z, Q = sample(spe, r, lag)
    ref, call = reference(r, lag, models, z, Q)
    got = run(r, lag, models, z, Q)
    check_parity("f64/33-steps", r, got, ref, call, 1e-9, "f64")
    before = snap(r.e)
    out = torch.full((n, r.e.S), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(spe.engine.UkfbError) as err:
        r.e.update_relative_dev(np.full(33, 0.05), slots, first, r.mu_hist, r.cov_hist, 32, 0, dev(r.e, np.where(np.isnan(z), 0.0, z)),
                                dev(r.e, Q.reshape(1, 36)), q_is_uniform=True, commit=True, mu_out=out, status=st)
    assert f"code {UKFB_ERR_OUT_OF_RANGE}" in str(err.value), str(err.value)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (st == -1).all() and same_snapshot(before, snap(r.e))
    r.e.close()


def test_orientation_engines_are_refused(spe):
    n = 8
    e = new_engine(spe, "orient", n, 0, 0)
    t = torch.float64
    hist_mu = torch.zeros((2, n, e.S), dtype=t, device="cuda")
    hist_cov = torch.zeros((2, n, e.PK), dtype=t, device="cuda")
    z, Q = torch.zeros((n, 7), dtype=t, device="cuda"), torch.zeros((36,), dtype=t, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(spe.engine.UkfbError) as err:
        e.update_relative_dev(np.array([0.05]), 2, 0, hist_mu, hist_cov, 1, 0, z, Q, q_is_uniform=True, commit=True, status=st)
    assert f"code {UKFB_ERR_WRONG_MODEL}" in str(err.value), str(err.value)
    torch.cuda.synchronize()
    assert (st == -1).all()
    e.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_host_array_form(spe, pname, prec, wide, tol):
    r = recorded(spe, pname)
    models, z, Q = sample(spe, r, MIXED)
    devf = run(r, MIXED, models, z, Q)
    mu, cov, a = window(r)
    o = r.e.update_relative(r.dt, mu, cov, MIXED, models, z, np.broadcast_to(Q, (N, 6, 6)), in_a=a, commit=False)
    assert (o["status"] == 0).all()
    for k in FLOATS:
        assert np.array_equal(o[k], devf[k]), k   # the same records in, the same kernel
