"""Late sensor-frame samples on the device (ukfb_update_delayed_sensor_dev / ukfb_update_delayed_sensor,
include/ukf_batch_delayed_sensor.h).

The history is recorded with history_push_dev during real cycles on the HOT inputs of tests/delayed_reference.py into a ring of 8
slots that the window of 6 steps wraps (first slot 5): tests/delayed_sensor_cases.py.  The reference is
tests/delayed_sensor_reference.py (pinned by tests/test_delayed_sensor_reference.py) run on the history and on the engine's state
AS DOWNLOADED, with inputs as the engine stores them.  Parity bound: |x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64) / 1e-4
(fp32) / 1e-9 + 2^-23 (fp32 engines with wide_arithmetic, against the reference's outputs rounded to fp32), and the scaled
per-block comparison of tests/feature_scaled_parity.py with that file's bounds (plain fp32: d_32 from
delayed_sensor_reference.delayed_sensor_f32).  The maxima measured on an MI355X are in profiles/delayed_sensor_parity.txt."""
import copy

import numpy as np
import pytest
import torch

import delayed_sensor_cases as dc
import delayed_sensor_reference as dsr
import feature_scaled_parity as fsp
import sensor_meas_reference as smr
import smoother_reference as sr
from engine_support import dev, host, same_snapshot, scaled_ignoring_nan, snapshot, stored, tdt, unpack
from probe_support import LDS_PATTERNS, lds_poison

pytestmark = pytest.mark.gpu

N = 1022   # not a multiple of four: the last workgroup holds two filters
STEPS, SLOTS, FIRST, PRECS = dc.STEPS, dc.SLOTS, dc.FIRST, dc.PRECS
ST_SKIPPED_SMALL_DT, ST_ERR_NEG_DT, ST_ERR_NONFINITE_MEAS, ST_ERR_CHOLESKY = 1 << 1, 1 << 2, 1 << 4, 1 << 5
ST_UNINITIALISED, ST_INACTIVE, ST_REJECTED_GATE = 1 << 7, 1 << 8, 1 << 9
UKFB_ERR_OUT_OF_RANGE, UKFB_ERR_WRONG_MODEL = 4, 5
OUT = ("mu_out", "cov_out", "z_pred", "S", "innov", "maha", "loglik")
IDENTITY = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def snap(e):
    """the engine's snapshot with the process noise of these filters"""
    return snapshot(e, range(min(e.capacity, 8)))


class Sample:
    """one late sample per filter: lag, ids, z, Q, mount, point, rate (None: the ring or the latch)"""


def window(r, mu_hist=None, cov_hist=None):
    mu = sr.window_order((r.mu_hist if mu_hist is None else mu_hist).double().cpu().numpy(), r.first, r.steps)
    cov = sr.window_order(unpack(host(r.cov_hist if cov_hist is None else cov_hist), r.e.D), r.first, r.steps)
    a = sr.window_order(r.in_a.double().cpu().numpy(), r.first, r.steps)
    b = sr.window_order(r.in_b.double().cpu().numpy(), r.first, r.steps)
    return mu, cov, a, b


def sample(spe, r, lag, ids=None, per_filter_q=False, rate=True, identity=False, one_mount=False):
    """the late sample of every filter, taken near the recorded state of its own step, inputs as the engine stores them;
    one_mount: the first filter's mount and point for the whole batch"""
    n, e = r.n, r.e
    s = Sample()
    s.lag = np.broadcast_to(np.asarray(lag), (n,)).astype(np.int32)
    s.ids = dc.cycling_ids(r.model, n) if ids is None else np.broadcast_to(np.asarray(ids), (n,)).astype(np.int32)
    mu_n = np.where(r.live[:, None], e.state(with_cov=False)[0], dc.dr.hot_initial(spe.synth, r.model, n)[0])
    mu = window(r)[0]
    mu_s = np.where(r.live[:, None], dc.state_at_lag(mu, mu_n, s.lag), mu_n)
    s.mount = stored(np.broadcast_to(smr.IDENTITY_MOUNT, (n, 7)) if identity else dc.mounts(n), e.dtype)
    s.point = stored(np.zeros((n, 3)) if identity else dc.points(r.model, n, mu_s), e.dtype)
    if one_mount:
        s.mount, s.point = np.broadcast_to(s.mount[0], (n, 7)).copy(), np.broadcast_to(s.point[0], (n, 3)).copy()
    s.rate = stored(dc.rates(n), e.dtype) if rate else None
    w = s.rate if rate else dsr.rate_source(s.lag, r.steps, None, window(r)[3], r.latch_b)
    s.z = stored(dc.samples(spe, r.model, s.ids, mu_s, s.mount, s.point, w), e.dtype)
    Q = np.broadcast_to(dc.Q_SAMPLE, (n, 3, 3))
    if per_filter_q:
        Q = Q * (1.0 + (np.arange(n) % 5) / 4.0)[:, None, None]
    s.Q = stored(Q if per_filter_q else dc.Q_SAMPLE, e.dtype)
    return s


def reference(spe, r, s, dt=None, rings=True, mu_hist=None, cov_hist=None, gate_chi2=-1.0):
    """-> (result dict of delayed_sensor_reference.update_delayed_sensor, the call's arguments for the fp32 evaluation)"""
    e = r.e
    mu, cov, a, b = window(r, mu_hist, cov_hist)
    if not rings:
        a, b = r.latch_a, r.latch_b
    if r.model == "pose":
        b = None
    mu_n, cov_n, _ = e.state()
    p = dc.params(spe, r)
    dt = (r.dt if dt is None else dt)[:r.steps - 1]
    w = np.zeros((r.n, 3)) if r.model == "pose" else dsr.rate_source(s.lag, r.steps, s.rate, b, r.latch_b)
    res = dsr.update_delayed_sensor(p, mu, cov, mu_n, cov_n, dt, s.lag, s.ids, s.z, s.Q, s.mount, s.point, rate=s.rate, latch_b=r.latch_b,
                                    in_a=a, in_b=b, initialised=r.live, gate_chi2=gate_chi2)
    return res, (p, mu, cov, mu_n, cov_n, dt, s.lag, s.ids, s.z, s.Q, s.mount, s.point, w, a, b)


def run(r, s, commit=False, dt=None, rings=True, mu_hist=None, cov_hist=None, outputs=True, uniform=()):
    """-> dict of NumPy arrays (float64; cov_out unpacked), and in ["raw"] the device tensors.  uniform: which of "lag", "ids",
    "mount", "point" go by value (the first filter's), not as arrays"""
    e, n = r.e, r.n
    t = tdt(e)
    per = lambda name, x: int(x[0]) if name in uniform else dev(e, np.asarray(x, dtype=np.int32), torch.int32)   # noqa: E731
    Q = np.asarray(s.Q, dtype=np.float64)
    uniform_q = Q.size == 9
    o = {}
    if outputs:
        nan = lambda *sh: torch.full(sh, float("nan"), dtype=t, device="cuda")   # noqa: E731
        o = dict(z_pred=nan(n, 4), S=nan(n, 9), innov=nan(n, 3), maha=nan(n), loglik=nan(n), mu_out=nan(n, e.S), cov_out=nan(n, e.PK),
                 status=torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    kw = dict(mount_dev=None if "mount" in uniform else dev(e, s.mount), mount=tuple(s.mount[0]) if "mount" in uniform else IDENTITY,
              point_dev=None if "point" in uniform else dev(e, s.point), point=tuple(s.point[0]) if "point" in uniform else (0.0, 0.0, 0.0),
              rate_dev=None if s.rate is None else dev(e, s.rate))
    e.update_delayed_sensor_dev((r.dt if dt is None else dt)[:r.steps - 1], r.slots, r.first, r.mu_hist if mu_hist is None else mu_hist,
                                r.cov_hist if cov_hist is None else cov_hist, per("lag", s.lag), per("ids", s.ids), dev(e, s.z),
                                dev(e, Q.reshape(-1, 9)), q_is_uniform=uniform_q, in_a_dev=r.in_a if rings else None,
                                in_b_dev=r.in_b if rings else None, commit=commit, **kw, **o)
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
    rows = ref["committed"] if rows is None else rows
    rnd = (lambda x: x.astype(np.float32).astype(np.float64)) if pname == "f32w" else (lambda x: x)
    assert np.array_equal(got["status"], ref["status"]), (name, np.unique(got["status"]), np.unique(ref["status"]))
    figs = {}
    for k in OUT:
        assert same_nan(got[k], ref[k]), (name, k)
        figs[k] = scaled_ignoring_nan(got[k], rnd(ref[k]))
    print(f"PARITY delayed_sensor/{name} n={r.n} " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()) + f" tol={tol:.3e}")
    for k, v in figs.items():
        assert v <= tol, (name, k, v, tol)
    if rows.any():
        p, mu, cov, mu_n, cov_n, dt, lag, ids, z, Q, mount, point, w, a, b = call

        def f32():
            i = np.nonzero(rows)[0]
            q = copy.copy(p)
            if np.ndim(q.R) == 3:
                q.R = q.R[i]
            QQ = np.broadcast_to(Q, (r.n, 3, 3))[i]
            aa = None if a is None else (a[:, i] if np.ndim(a) == 3 else a[i])
            bb = None if b is None else (b[:, i] if np.ndim(b) == 3 else b[i])
            return tuple(dsr.delayed_sensor_f32(q, mu[:, i], cov[:, i], mu_n[i], cov_n[i], dt, lag[i], ids[i], z[i], QQ, mount[i], point[i], w[i],
                                                aa, bb, prec=pr) for pr in ("f32", "f64"))
        fsp.judge_state("delayed_sensor/" + name, r.model, pname, got["mu_out"][rows], got["cov_out"][rows], ref["mu_out"][rows],
                        ref["cov_out"][rows], f32=f32)
    return figs


_CACHE = {}


def recorded(spe, model, pname, n=N):
    """a recording that the tests which commit nothing share"""
    key = (model, pname, n)
    if key not in _CACHE:
        _, prec, wide, _ = [p for p in PRECS if p[0] == pname][0]
        _CACHE[key] = dc.record(spe, model, n, prec, wide)
    return _CACHE[key]


MIXED = np.arange(N) % STEPS   # lags 0 ... 5: the four rows of a wavefront differ


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_parity_commit_modes_and_outputs(spe, model, pname, prec, wide, tol):
    """1. mixed lags, the engine's models cycling, per-filter mounts with a non-trivial qs, per-filter points, Q per filter and
    uniform (half of the runs each); commit = 0 keeps every bit of the engine; commit = 1 with out = NULL stores commit = 0's mu_out / cov_out bit for
    bit.  Runs on a fresh recording: it commits."""
    r = dc.record(spe, model, N, prec, wide)
    r.e.set_last_measurement_time(np.arange(1, N + 1, dtype=np.int64) * 1000 + 7)
    before = snap(r.e)
    per_filter_q = (pname != "f32") == (model == "pose")   # half of the six runs
    s = sample(spe, r, MIXED, per_filter_q=per_filter_q)
    ref, call = reference(spe, r, s)
    assert (ref["status"] == 0).all() and ref["committed"].all()   # no filter is silently left out
    got = run(r, s, commit=False)
    assert same_snapshot(before, snap(r.e)), "commit = 0 changed the engine"
    check_parity(f"{model}/{pname}/{'Q-per-filter' if per_filter_q else 'Q-uniform'}", r, got, ref, call, tol, pname)
    m = np.array([smr.meas_dim(int(i)) for i in s.ids])
    assert (got["z_pred"][:, 3] == 0).all() and (got["z_pred"][m == 1, 1:] == 0).all()
    run(r, s, commit=True, outputs=False)
    after = snap(r.e)
    assert np.array_equal(after[0], got["mu_out"]) and np.array_equal(after[1], got["cov_out"])
    assert (after[3] == 0).all() and all(np.array_equal(x, y) for x, y in zip(before[4:6], after[4:6]))   # times and noise stay
    r.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_lag_zero_is_the_sensor_frame_update(spe, model, pname, prec, wide, tol):
    """2. against ukfb_update_sensor_dev on a twin engine, within the parity tolerance (M = I only to rounding: no bit identity)"""
    n = 254
    r, twin = dc.record(spe, model, n, prec, wide), dc.record(spe, model, n, prec, wide)
    s = sample(spe, r, 0, rate=False)
    got = run(r, s)
    e = twin.e
    e.update_sensor_dev(0, dev(e, s.z), dev(e, np.broadcast_to(s.Q.reshape(1, 9), (n, 9))), model_dev=dev(e, s.ids, torch.int32),
                        mount_dev=dev(e, s.mount), point_dev=dev(e, s.point))
    mu_t, cov_t, _ = e.state()
    assert (got["status"] == 0).all() and (e.status() == 0).all()
    em, ec = scaled_ignoring_nan(got["mu_out"], mu_t), scaled_ignoring_nan(got["cov_out"], cov_t)
    print(f"PARITY delayed_sensor/{model}/{pname}/lag-0 against update_sensor_dev: mu {em:.3e} cov {ec:.3e} tol={tol:.3e}")
    assert em <= tol and ec <= tol
    r.e.close(); twin.e.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_identity_mount_is_the_delayed_update_with_model_0(spe, pname, prec, wide, tol):
    """3. POSE_POSITION with r = 0 against ukfb_update_delayed_dev, model 0, on the same recording with mixed lags"""
    r = recorded(spe, "pose", pname)
    s = sample(spe, r, MIXED, ids=smr.POSE_POSITION, identity=True)
    got = run(r, s, uniform=("mount", "point"))
    e, t = r.e, tdt(r.e)
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=t, device="cuda")   # noqa: E731
    o = dict(mu_out=nan(N, e.S), cov_out=nan(N, e.PK), maha=nan(N), status=torch.full((N,), -1, dtype=torch.int32, device="cuda"))
    e.update_delayed_dev(r.dt, SLOTS, FIRST, r.mu_hist, r.cov_hist, dev(e, s.lag, torch.int32), 0, dev(e, s.z), dev(e, s.Q.reshape(1, 9)),
                         q_is_uniform=True, in_a_dev=r.in_a, in_b_dev=r.in_b, commit=False, **o)
    torch.cuda.synchronize()
    assert (got["status"] == 0).all() and (o["status"].cpu().numpy() == 0).all()
    figs = {"mu_out": scaled_ignoring_nan(got["mu_out"], host(o["mu_out"])),
            "cov_out": scaled_ignoring_nan(got["cov_out"], unpack(host(o["cov_out"]), e.D)), "maha": scaled_ignoring_nan(got["maha"], host(o["maha"]))}
    print(f"PARITY delayed_sensor/pose/{pname}/identity-mount against update_delayed_dev model 0: " +
          " ".join(f"{k}={v:.3e}" for k, v in figs.items()) + f" tol={tol:.3e}")
    assert max(figs.values()) <= tol


def test_rate_source_of_model_5(spe):
    """4. ORIENT_VELOCITY reads rate_dev, else the rotation-rate ring at the sample's step, else the latch: each against the
    reference fed that rate, and the three results differ"""
    n = 254
    r = recorded(spe, "orient", "f64", n)
    lag = 1 + np.arange(n) % (STEPS - 1)
    outs = []
    for name, rate, rings in (("rate_dev", True, True), ("ring", False, True), ("latch", False, False)):
        s = sample(spe, r, lag, ids=smr.ORIENT_VELOCITY, rate=True)   # the same sample in all three runs
        if not rate:
            s.rate = None
        ref, call = reference(spe, r, s, rings=rings)
        assert (ref["status"] == 0).all() and ref["committed"].all()
        got = run(r, s, rings=rings)
        check_parity(f"orient/f64/model-5/{name}", r, got, ref, call, 1e-9, "f64")
        outs.append(got["mu_out"])
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert scaled_ignoring_nan(outs[i], outs[j]) > 1e-6, (i, j)


def quiet_rows(spe, r, model, n, gate=False):
    """the rows of the CPU status test among healthy wave-mates -> (clean sample, the sample with the rows planted, poisoned
    rings, the quiet filters, the statuses they must show)"""
    lag = np.arange(n) % STEPS
    clean = sample(spe, r, lag)
    s = sample(spe, r, lag)
    other = smr.ORIENT_VELOCITY if model == "pose" else smr.POSE_POSITION
    s.lag, s.ids, s.z, s.mount, s.point, s.rate = (x.copy() for x in (s.lag, s.ids, s.z, s.mount, s.point, s.rate))
    s.lag[1], s.lag[2], s.lag[3] = STEPS, 1000, -1
    s.ids[5], s.ids[6], s.ids[7] = -1, other, 8
    s.z[9, 0] = np.nan
    lever = smr.POSE_POSITION if model == "pose" else smr.ORIENT_VELOCITY
    nolever = smr.POSE_NAV_VELOCITY if model == "pose" else smr.ORIENT_SPECIFIC_FORCE
    s.ids[10], s.ids[17] = lever, nolever
    if gate:
        s.lag[17] = 0   # (the sample is drawn near the FILTERED record of its step; under a gate of 9 only the present is near enough)
    s.mount[10, 1] = np.inf
    s.mount[17], s.point[17], s.rate[17], s.z[17] = np.nan, np.nan, np.nan, clean_z(spe, r, s, 17)   # unread entries: healthy
    # poisoned history records inside the chains of filters 13 (a non-positive covariance) and 14 (a NaN in the mean); filter 15
    # has the same poison BELOW its chain and stays healthy
    s.lag[13], s.lag[14], s.lag[15] = 3, 4, 1
    for i in (13, 14, 15):
        s.ids[i] = clean.ids[0]
        s.z[i] = clean_z(spe, r, s, i)
    ch, mh = r.cov_hist.clone(), r.mu_hist.clone()
    D = r.e.D
    ind = torch.from_numpy(-np.eye(D)[np.tril_indices(D)]).to("cuda", ch.dtype)
    ch[(FIRST + 3) % SLOTS, 13] = ind
    mh[(FIRST + 2) % SLOTS, 14, 1] = float("nan")
    ch[(FIRST + 1) % SLOTS, 15] = ind
    want = {1: ST_ERR_NEG_DT, 2: ST_ERR_NEG_DT, 3: ST_INACTIVE, 5: ST_INACTIVE, 6: ST_INACTIVE, 7: ST_INACTIVE, 9: ST_ERR_NONFINITE_MEAS,
            10: ST_ERR_NONFINITE_MEAS, 13: ST_ERR_CHOLESKY, 14: ST_ERR_CHOLESKY, 15: 0, 17: 0}
    if gate:
        s.z[21] = s.z[21] + 40.0
        want[21] = ST_REJECTED_GATE
    return clean, s, mh, ch, want


def clean_z(spe, r, s, i):
    """the sample of filter i for the model, lag and inputs `s` now gives it (unread inputs may be NaN: they are neutralised)"""
    mu_n = r.e.state(with_cov=False)[0]
    mu_s = dc.state_at_lag(window(r)[0], mu_n, s.lag)
    _, _, um, up = smr.used_inputs(int(s.ids[i]))
    mount = np.where(um, s.mount[i], smr.IDENTITY_MOUNT)[None]
    point = np.where(up, s.point[i], 0.0)[None]
    w = np.zeros((1, 3)) if int(s.ids[i]) != smr.ORIENT_VELOCITY else s.rate[i][None]
    m = smr.meas_dim(int(s.ids[i]))
    z = np.zeros(3)
    z[:m] = smr.h(int(s.ids[i]), mu_s[i][None], mount, point, w)[0] + 0.05
    return stored(z, r.e.dtype)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_filters_that_commit_nothing_keep_every_bit(spe, model):
    """5. the CPU status rows among healthy wave-mates"""
    n, dead = 64, 22
    r = dc.record(spe, model, n, 0, 0, skip_init=(dead,))
    clean_s, s, mh, ch, want = quiet_rows(spe, r, model, n)
    clean = run(r, clean_s)
    ref, _ = reference(spe, r, s, mu_hist=mh, cov_hist=ch)
    before = snap(r.e)
    got = run(r, s, mu_hist=mh, cov_hist=ch)
    st = got["status"]
    assert np.array_equal(st, ref["status"]), (st, ref["status"])
    for i, w in want.items():
        assert st[i] == w, (i, st[i], w)
    assert st[dead] == ST_UNINITIALISED
    quiet = np.array([i for i, w in want.items() if w != 0] + [dead])
    for k in OUT:
        assert np.isnan(got[k][quiet]).all(), k
    # wave-mates: the bits of the run in which everybody is healthy -- their own lag, model and sample are unchanged
    same = np.ones(n, bool)
    same[quiet] = False
    same[[15, 17]] = False
    for k in OUT + ("status",):
        assert np.array_equal(got[k][same], clean[k][same]), k
    for i in (15, 17):
        assert scaled_ignoring_nan(got["mu_out"][i], ref["mu_out"][i]) <= 1e-9 and scaled_ignoring_nan(got["cov_out"][i], ref["cov_out"][i]) <= 1e-9
    # committing: the quiet filters keep every bit of the engine, the others store mu_out
    run(r, s, mu_hist=mh, cov_hist=ch, commit=True, outputs=False)
    after = snap(r.e)
    assert np.array_equal(after[0][quiet], before[0][quiet], equal_nan=True) and np.array_equal(after[1][quiet], before[1][quiet], equal_nan=True)
    keep = np.ones(n, bool)
    keep[quiet] = False
    assert np.array_equal(after[0][keep], got["mu_out"][keep]) and np.array_equal(after[1][keep], got["cov_out"][keep])
    assert np.array_equal(after[3], st), "commit = 1 writes the call's status to the engine's array"
    r.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_gate_rejects_with_outputs_written(spe, model):
    """6. gate_chi2 = 9, every second sample far off"""
    n = 64
    r = dc.record(spe, model, n, 0, 0, gate_chi2=9.0)
    s = sample(spe, r, 2)
    s.z = s.z.copy()
    s.z[::2, 0] += 40.0
    ref, _ = reference(spe, r, s, gate_chi2=9.0)
    before = snap(r.e)
    got = run(r, s, commit=True)
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
    """7. per-filter process noise, ring inputs against latched inputs, a gated dt in the middle of the window"""
    n = 254
    r = dc.record(spe, model, n, prec, wide, per_filter_noise=True)
    lag = np.arange(n) % STEPS
    s = sample(spe, r, lag)
    outs = {}
    for rings in (True, False):
        ref, call = reference(spe, r, s, rings=rings)
        outs[rings] = run(r, s, rings=rings)
        check_parity(f"{model}/{pname}/per-filter-noise/{'rings' if rings else 'latches'}", r, outs[rings], ref, call, tol, pname)
    assert not np.array_equal(outs[True]["mu_out"], outs[False]["mu_out"])
    dt = r.dt.copy()
    dt[2] = 0.0   # the prediction 2 -> 3: inside the chains of lags 3, 4, 5
    ref, call = reference(spe, r, s, dt=dt)
    got = run(r, s, dt=dt)
    assert (got["status"][lag >= 3] == ST_SKIPPED_SMALL_DT).all() and (got["status"][lag < 3] == 0).all()
    check_parity(f"{model}/{pname}/gated-dt", r, got, ref, call, tol, pname)
    r.e.close()


def test_largest_window_and_one_step_more(spe):
    """8. 33 steps with lag 32 on 130 filters (a ring of 40 that the window wraps); 34 steps: OUT_OF_RANGE, nothing written"""
    steps, slots, first, n = 33, 40, 20, 130
    r = dc.record(spe, "pose", n, 0, 0, steps=steps, slots=slots, first=first)
    lag = np.where(np.arange(n) % 4 == 3, 17, 32)
    s = sample(spe, r, lag)
    ref, call = reference(spe, r, s)
    got = run(r, s)
    check_parity("pose/f64/33-steps", r, got, ref, call, 1e-9, "f64")
    before = snap(r.e)
    out = torch.full((n, r.e.S), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(spe.engine.UkfbError) as err:
        r.e.update_delayed_sensor_dev(np.full(33, 0.05), slots, first, r.mu_hist, r.cov_hist, 32, 0, dev(r.e, s.z), dev(r.e, s.Q.reshape(1, 9)),
                                      q_is_uniform=True, commit=True, mu_out=out, status=st)
    assert f"code {UKFB_ERR_OUT_OF_RANGE}" in str(err.value), str(err.value)
    # a uniform id of the other engine is refused too, and writes nothing
    with pytest.raises(spe.engine.UkfbError) as err:
        r.e.update_delayed_sensor_dev(r.dt, slots, first, r.mu_hist, r.cov_hist, 32, smr.ORIENT_VELOCITY, dev(r.e, s.z),
                                      dev(r.e, s.Q.reshape(1, 9)), q_is_uniform=True, commit=True, mu_out=out, status=st)
    assert f"code {UKFB_ERR_WRONG_MODEL}" in str(err.value), str(err.value)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (st == -1).all() and same_snapshot(before, snap(r.e))
    r.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_host_array_form(spe, model, pname, prec, wide, tol):
    """9. bit-equal to the device form on the same records"""
    r = recorded(spe, model, pname)
    s = sample(spe, r, MIXED, per_filter_q=True)
    devf = run(r, s)
    mu, cov, a, b = window(r)
    o = r.e.update_delayed_sensor(r.dt, mu, cov, s.lag, s.ids, s.z, s.Q, mount=s.mount, point=s.point, rate=s.rate, in_a=a, in_b=b, commit=False)
    assert (o["status"] == 0).all()
    for k in OUT:
        assert np.array_equal(o[k], devf[k]), k   # the same records in, the same kernel


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_uniform_forms_are_the_arrays_bit_for_bit(spe, model):
    """10. a uniform id, mount, point, Q and lag against the same values given as arrays"""
    r = recorded(spe, model, "f64")
    s = sample(spe, r, 3, ids=smr.POSE_POINT if model == "pose" else smr.ORIENT_VELOCITY, one_mount=True)
    a = run(r, s, uniform=("lag", "ids", "mount", "point"))
    s.Q = np.broadcast_to(s.Q, (N, 3, 3)).copy()
    b = run(r, s)
    assert (a["status"] == 0).all()
    for k in OUT + ("status",):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_lds_leftovers(spe, model, pname, prec, wide, tol):
    """11. 253 filters with an uninitialised, a failing, an inactive, a non-finite and a gated row among healthy wave-mates: once
    un-poisoned and once after each pattern of tests/probe_support.py, applied right before the call; every output and the
    snapshot bit-equal (the method of tests/test_gpu_feature_lds_leftovers.py)"""
    n, dead = 253, 22
    r = dc.record(spe, model, n, prec, wide, skip_init=(dead,), gate_chi2=9.0)
    _, s, mh, ch, want = quiet_rows(spe, r, model, n, gate=True)
    poison = lds_poison()
    runs = []
    for commit in (False, True):   # (the committing run last: the read-only ones leave the engine as it is)
        for pat in ((None,) + LDS_PATTERNS) if not commit else (LDS_PATTERNS[0],):
            before = snap(r.e)
            torch.cuda.synchronize()
            if pat is not None:
                assert poison(pat) == 0
            got = run(r, s, mu_hist=mh, cov_hist=ch, commit=commit)
            runs.append((pat, got, before, snap(r.e)))
    _, got0, before0, _ = runs[0]
    st = got0["status"]
    for i, w in want.items():
        assert st[i] == w, (i, st[i], w)
    assert st[dead] == ST_UNINITIALISED and (st == 0).sum() > 0.8 * n and np.isfinite(got0["mu_out"][st == 0]).all()
    for pat, got, before, after in runs[1:]:
        differ = [k for k in OUT + ("status",) if not np.array_equal(got[k], got0[k], equal_nan=True)]
        assert not differ, (hex(pat), differ)
        assert same_snapshot(before, before0), hex(pat)
    for pat, got, before, after in runs[:-1]:
        assert same_snapshot(before, after), "a read-only run changed the engine"
    after = runs[-1][3]
    ok = st == 0
    assert np.array_equal(after[0][ok], got0["mu_out"][ok]) and np.array_equal(after[0][~ok], before0[0][~ok], equal_nan=True)
    r.e.close()
