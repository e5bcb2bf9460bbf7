"""Forecast on the device (ukfb_forecast_dev / ukfb_forecast, include/ukf_batch.h): `steps` predictions chained from a start
record into rings of the history's format, read-only on the engine.

The engines have been cycled a few times (Pose: the acceleration branch with POS3 updates; OrientationState: its body-velocity
update; inputs from synth), so their covariances are full.  The input rings hold synth's inputs of the following cycles, Pose
with every fifth filter on a NaN acceleration row.  The reference is tests/forecast_reference.py (pinned by
tests/test_forecast_reference.py) run on the start record and the inputs AS DOWNLOADED, so that storage rounding of the inputs
is out of the comparison.  Parity bound: |x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64) / 1e-4 (fp32) / 1e-9 + 2^-23 (fp32
engines with wide_arithmetic, against the reference's outputs rounded to fp32).  The maxima measured on an MI355X are in
profiles/forecast_parity.txt.

Every parity comparison also makes the SCALED one (tests/feature_scaled_parity.py) over every step: fp64 1e-9;
wide_arithmetic 2 u v + 1e-9; plain fp32 max(M_feat d_32, 20 u v), d_32 the distance of the all-float32 evaluation of the same
call (forecast_reference.forecast(prec="f32")) from its float64 evaluation.  The chain is never narrowed below the arithmetic
type between steps (CSM / CSP of ukf_forecast.hpp), so every step's record is one rounding from the chain: c = 1 for every
step, whatever the horizon."""
import ctypes as C

import numpy as np
import pytest
import torch

import feature_scaled_parity as fsp
import forecast_reference as fr
import smoother_reference as sr
from engine_support import host, new_engine, same_snapshot, scaled, snapshot, tdt, unpack

pytestmark = pytest.mark.gpu

N = 1022   # not a multiple of four: the last workgroup holds two filters
STEPS, SLOTS, FIRST = 6, 8, 5
PRECS = [("f64", 0, 0, 1e-9), ("f32", 1, 0, 1e-4), ("f32w", 1, 1, 1e-9 + 2.0 ** -23)]
IDS = [p[0] for p in PRECS]
ACC_COV = 0.01 * np.eye(3)
CYCLES = 3
ST_SKIPPED_FIRST_TS, ST_SKIPPED_SMALL_DT, ST_ERR_NEG_DT, ST_ERR_CHOLESKY, ST_UNINITIALISED = 1, 1 << 1, 1 << 2, 1 << 5, 1 << 7


class Setup:
    """a cycled engine, the input rings of a horizon on the device, and everything as the host saw it"""


def latch(e, model, a, b):
    if model == "pose":
        e.set_acceleration(a, ACC_COV)
    else:
        e.set_orient_inputs(b, a)


def setup(spe, model, n, prec, wide, steps=STEPS, slots=SLOTS, first=FIRST, skip_init=(), per_filter_noise=False, **kw):
    sy = spe.synth
    e = new_engine(spe, model, n, prec, wide, **kw)
    if per_filter_noise:   # every filter its own matrix (x1 ... x2.5, every third one half as much again): Rn and Racc are strided
        scale = 1.0 + np.arange(n) / n + 0.5 * (np.arange(n) % 3 == 0)
        e.set_process_noise(scale[:, None, None] * e.process_noise()[None])
    mu0, cov0 = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
    live = np.ones(n, bool)
    live[list(skip_init)] = False
    for i in np.nonzero(live)[0] if skip_init else ():
        e.initialize(mu0[i:i + 1], cov0[i:i + 1], first=int(i))
    if not skip_init:
        e.initialize(mu0, cov0)

    def inputs(c, mu_now):
        if model == "pose":
            acc, z, Q = sy.pose_cycle_inputs(n, c, mu_now[:, :3])
            return acc, np.zeros((n, 3)), z, Q
        gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu_now[:, 0:4])
        return acc, gyro, z, Q
    for c in range(CYCLES):
        a, b, z, Q = inputs(c, e.state(with_cov=False)[0])
        latch(e, model, a, b)
        e.cycle(0.01, spe.MEAS_POS3 if model == "pose" else spe.MEAS_ORIENT_BODYVEL3, z, Q)
    s = Setup()
    s.e, s.model, s.n, s.steps, s.slots, s.first, s.live, s.per_filter_noise = e, model, n, steps, slots, first, live, per_filter_noise
    mu_now = e.state(with_cov=False)[0]
    s.in_a = torch.zeros((slots, n, 3), dtype=tdt(e), device="cuda")
    s.in_b = torch.zeros((slots, n, 3), dtype=tdt(e), device="cuda")
    s.host_a, s.host_b = [], []
    for c in range(steps):
        a, b, _, _ = inputs(CYCLES + c, mu_now)
        if model == "pose":
            a[::5] = np.nan   # the constant-velocity branch
        slot = (first + c) % slots
        s.in_a[slot] = torch.from_numpy(a).to("cuda", tdt(e))
        s.in_b[slot] = torch.from_numpy(b).to("cuda", tdt(e))
        s.host_a.append(a); s.host_b.append(b)
    # what the engine's own latches hold from here on, as stored
    a, b, _, _ = inputs(CYCLES - 1, mu_now)
    latch(e, model, a, b)
    s.latch_a, s.latch_b = a.astype(e.dtype).astype(np.float64), b.astype(e.dtype).astype(np.float64)
    s.dt = np.array([0.01 * (1.0 + 0.1 * (c % 7)) for c in range(steps)])
    return s


def params(spe, s):
    e, sy = s.e, spe.synth
    R = np.array([e.process_noise(i) for i in range(s.n)]) if s.per_filter_noise else e.process_noise()
    R = np.asarray(R, dtype=e.dtype).astype(np.float64)
    if s.model == "pose":
        return sr.Params("pose", R, acc_cov=np.asarray(2.0 * ACC_COV, dtype=e.dtype).astype(np.float64) / 2.0)
    from oracle import ukf_numpy as on
    return sr.Params("orient", R, tau_g=sy.ORIENT_TAU, tau_a=sy.ORIENT_TAU, earth=on.earth_rotation(sy.ORIENT_LATITUDE))


class Reference(tuple):
    """the result of forecast_reference.forecast, and in .call the keywords it was called with (for its fp32 evaluation)"""

    def __new__(cls, result, call):
        self = super().__new__(cls, result)
        self.call = call
        return self


def reference(spe, s, start=None, dt=None, ts_us=None, steps=None, first=None, rings=True):
    """on the start record (default: the engine's state) and the inputs as downloaded"""
    e = s.e
    steps = s.steps if steps is None else steps
    first = s.first if first is None else first
    if start is None:
        mu, cov, _ = e.state()
    else:
        mu, cov = start[0].double().cpu().numpy(), unpack(host(start[1]), e.D)
    a = sr.window_order(s.in_a.double().cpu().numpy(), first, steps)
    b = sr.window_order(s.in_b.double().cpu().numpy(), first, steps)
    if not rings:
        a, b = s.latch_a, s.latch_b
    kw = dict(in_a=a, in_b=b if s.model == "orient" else None, initialised=s.live)
    if ts_us is not None:
        kw.update(ts_us=np.asarray(ts_us)[:steps], last_us=e.last_measurement_time())
    else:
        kw.update(dt=(s.dt if dt is None else dt)[:steps])
    call = (params(spe, s), mu, cov, kw)
    return Reference(fr.forecast(call[0], mu, cov, **kw), call)


def rings_like(s, cov=True):
    e = s.e
    mo = torch.full((s.slots, s.n, e.S), float("nan"), dtype=tdt(e), device="cuda")
    co = torch.full((s.slots, s.n, e.PK), float("nan"), dtype=tdt(e), device="cuda") if cov else None
    return mo, co


def run(s, dt=None, ts_us=None, steps=None, first=None, start=None, cov=True, rings=True, out=None):
    """-> (mu [steps, n, S], cov [steps, n, D, D] or None, status [n], (mu ring, cov ring)) in window order"""
    e = s.e
    steps = s.steps if steps is None else steps
    first = s.first if first is None else first
    mo, co = rings_like(s, cov) if out is None else out
    st = torch.full((s.n,), -1, dtype=torch.int32, device="cuda")
    kw = dict(ts_us=np.asarray(ts_us)[:steps]) if ts_us is not None else dict(dt=(s.dt if dt is None else dt)[:steps])
    e.forecast_dev(s.slots, first, mo, co, st, start_mu=None if start is None else start[0],
                   start_cov=None if start is None else start[1], in_a_dev=s.in_a if rings else None,
                   in_b_dev=s.in_b if rings else None, **kw)
    torch.cuda.synchronize()
    mu_f = sr.window_order(mo.double().cpu().numpy(), first, steps)
    cov_f = sr.window_order(unpack(host(co), e.D), first, steps) if co is not None else None
    return mu_f, cov_f, st.cpu().numpy().astype(np.uint32), (mo, co)


def run_chained(s, chunk):
    """the horizon in calls of `chunk` steps, each started through start_*_dev from the last slot of the call before (a slot of
    the same rings outside the call's window) -> (mu, cov, status OR) in window order"""
    out, start, st = rings_like(s), None, np.zeros(s.n, np.uint32)
    for c0 in range(0, s.steps, chunk):
        part = run(s, dt=s.dt[c0:c0 + chunk], steps=chunk, first=(s.first + c0) % s.slots, start=start, out=out)
        st |= part[2]
        prev = (s.first + c0 + chunk - 1) % s.slots
        start = (out[0][prev], out[1][prev])
    return (sr.window_order(out[0].double().cpu().numpy(), s.first, s.steps), sr.window_order(unpack(host(out[1]), s.e.D), s.first, s.steps), st)


def check_parity(name, s, got, ref, tol, wide, rows=slice(None)):
    """the file's bound, then the scaled check of every step (tests/feature_scaled_parity.py)"""
    mu_f, cov_f = got[0], got[1]
    mu_r, cov_r = ref[0], ref[1]
    if wide:   # the engine stores fp32
        mu_r, cov_r = mu_r.astype(np.float32).astype(np.float64), cov_r.astype(np.float32).astype(np.float64)
    em, ec = scaled(mu_f[:, rows], mu_r[:, rows]), scaled(cov_f[:, rows], cov_r[:, rows])
    print(f"PARITY {name} n={s.n} steps={mu_f.shape[0]} max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e} tol={tol:.3e}")
    assert em <= tol and ec <= tol, (name, em, ec, tol)
    mode = "wide" if wide else ("f64" if s.e.dtype == np.float64 else "f32")
    p, mu, cov, kw = ref.call
    pick = np.zeros(mu_f.shape[:2], bool)
    pick[:, rows] = True
    kw = dict(kw, initialised=None)

    def f32():
        return tuple(fr.forecast(p, mu, cov, prec=q, **kw)[:2] for q in ("f32", "f64"))
    fsp.judge_state("forecast/" + name, s.model, mode, mu_f, cov_f, ref[0], ref[1], f32=f32, rows=pick.reshape(-1))


_CACHE = {}


def cycled(spe, model, pname):
    key = (model, pname)
    if key not in _CACHE:
        _, prec, wide, _ = [p for p in PRECS if p[0] == pname][0]
        s = setup(spe, model, N, prec, wide)
        _CACHE[key] = (s, reference(spe, s))
    return _CACHE[key]


def start_record(s):
    """the engine's state as device tensors of the engine's format (a caller's start record)"""
    e = s.e
    mu, cov, _ = e.state()
    il = np.tril_indices(e.D)
    return (torch.from_numpy(mu).to("cuda", tdt(e)), torch.from_numpy(np.ascontiguousarray(cov[:, il[0], il[1]])).to("cuda", tdt(e)))


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=IDS)
def test_parity_six_steps(spe, model, pname, prec, wide, tol):
    """6 steps in a ring of 8 that the window wraps (first slot 5), N = 1022, varying dt, input rings"""
    s, ref = cycled(spe, model, pname)
    got = run(s)
    assert (ref[2] == 0).all()
    assert (got[2] == 0).all(), np.unique(got[2])
    check_parity(f"{model}/{pname}", s, got, ref, tol, wide)
    # slots outside the window keep the sentinel
    outside = [k for k in range(SLOTS) if k not in [(FIRST + c) % SLOTS for c in range(STEPS)]]
    assert torch.isnan(got[3][0][outside]).all() and torch.isnan(got[3][1][outside]).all()
    if model == "pose":   # both branches are in the batch
        assert torch.isnan(s.in_a[FIRST, ::5]).all() and torch.isfinite(s.in_a[FIRST, 1::5]).all()


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=IDS)
@pytest.mark.parametrize("steps,n,slots,first", [(12, 203, 16, 9), (32, 64, 32, 7)], ids=["12-steps", "32-steps"])
def test_parity_long_chain(spe, model, pname, prec, wide, tol, steps, n, slots, first):
    """12 steps in a ring of 16 that the window wraps, and the cap: 32 steps in a ring of 32"""
    s = setup(spe, model, n, prec, wide, steps=steps, slots=slots, first=first)
    got, ref = run(s), reference(spe, s)
    assert (ref[2] == 0).all()
    assert (got[2] == 0).all(), np.unique(got[2])
    assert got[0].shape[0] == steps
    check_parity(f"{model}/{pname}/{steps}-steps", s, got, ref, tol, wide)
    s.e.close()


def test_thirty_three_steps_are_out_of_range_and_write_nothing(spe):
    s = setup(spe, "pose", 64, 0, 0, steps=4, slots=40, first=0)
    e = s.e
    mo = torch.full((40, 64, e.S), float("nan"), dtype=torch.float64, device="cuda")
    co = torch.full((40, 64, e.PK), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    dt = (C.c_double * 33)(*([0.01] * 33))
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    stp = C.cast(st.data_ptr(), C.POINTER(C.c_uint32))   # the header's uint32_t* status_dev
    args = (C.c_int(40), C.c_int(0), None, None, None, None, ptr(mo), ptr(co), stp)
    assert e._lib.ukfb_forecast_dev(e._h, C.c_int(33), dt, None, *args) == 4   # UKFB_ERR_OUT_OF_RANGE
    with pytest.raises(spe.engine.UkfbError):
        e.forecast_dev(40, 0, mo, co, st, dt=np.full(33, 0.01))
    torch.cuda.synchronize()
    assert torch.isnan(mo).all() and torch.isnan(co).all() and (st == -1).all()
    assert e._lib.ukfb_forecast_dev(e._h, C.c_int(32), dt, None, *args) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(mo[:32]).all() and torch.isnan(mo[32:]).all() and (st == 0).all()
    # exactly one start pointer is an invalid argument
    assert e._lib.ukfb_forecast_dev(e._h, C.c_int(2), dt, None, C.c_int(40), C.c_int(0), ptr(mo), None, None, None, ptr(mo), ptr(co),
                                    stp) == 1
    e.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS[:2], ids=IDS[:2])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_parity_latched_inputs_and_per_filter_noise(spe, model, pname, prec, wide, tol):
    """NULL input rings (the engine's latches, held over the horizon) and a process noise per filter (strided Rn and, Pose,
    Racc)"""
    s = setup(spe, model, 254, prec, wide, per_filter_noise=True)
    for rings in (True, False):
        got, ref = run(s, rings=rings), reference(spe, s, rings=rings)
        assert (got[2] == 0).all() and (ref[2] == 0).all()
        check_parity(f"{model}/{pname}/per-filter-noise/{'rings' if rings else 'latches'}", s, got, ref, tol, wide)
    s.e.close()


def pair(spe, model, n, prec, wide, **kw):
    """two engines with the same history"""
    a, b = setup(spe, model, n, prec, wide, **kw), setup(spe, model, n, prec, wide, **kw)
    assert same_snapshot(snapshot(a.e), snapshot(b.e))
    return a, b


def report_twin(name, got, twin_mu, twin_cov, tol):
    em, ec = scaled(got[0], twin_mu), scaled(got[1], twin_cov)
    same = np.array_equal(got[0], twin_mu) and np.array_equal(got[1], twin_cov)
    print(f"TWIN {name} bit_identical={same} max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e} tol={tol:.3e}")
    assert em <= tol and ec <= tol, (name, em, ec)


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=IDS)
def test_twin_makes_the_same_predictions(spe, model, pname, prec, wide, tol):
    """a twin engine with the same history makes the same `steps` calls of ukfb_predict, latching each step's inputs first.
    Bits are reported, not asserted: the forward kernel's summation order is its own.

    fp64 and plain fp32: ONE call over the horizon.  wide_arithmetic: the horizon in one-step calls chained through
    start_*_dev.  There the twin is another computation than the one call: every ukfb_predict narrows the twin's state to fp32,
    the one call keeps its chain in fp64 (include/ukf_batch.h), so the two differ by up to `steps` fp32 roundings, carried
    along, where the file's wide bound allows the one rounding of a store -- measured on an MI355X at 6 steps: Pose 1.9e-7 in
    the mean against 1e-9 + 2^-23 = 1.2e-7.  The one-step calls narrow every record as the twin does and are held to the bound;
    the one call's figure is printed beside it.  The one call's chain in wide mode is held to the reference in the parity
    tests above, 32 steps included."""
    n = 130
    s, t = pair(spe, model, n, prec, wide)
    got = run(s)
    one_call = got
    if wide:
        got = run_chained(s, 1)
    mh, ch = rings_like(t)
    st = np.zeros(n, np.uint32)
    for c in range(STEPS):
        latch(t.e, model, t.host_a[c], t.host_b[c])
        t.e.predict(float(t.dt[c]))
        st |= t.e.status()
        t.e.history_push_dev(SLOTS, (FIRST + c) % SLOTS, mh, ch)
    t.e.sync()
    twin_mu, twin_cov = sr.window_order(mh.double().cpu().numpy(), FIRST, STEPS), sr.window_order(unpack(host(ch), t.e.D), FIRST, STEPS)
    if wide:
        print(f"TWIN {model}/{pname}/dt one call (chain in fp64, not asserted): max_scaled_dmu={scaled(one_call[0], twin_mu):.3e} "
              f"max_scaled_dcov={scaled(one_call[1], twin_cov):.3e}")
    report_twin(f"{model}/{pname}/dt" + ("/one-step calls" if wide else ""), got, twin_mu, twin_cov, tol)
    assert np.array_equal(got[2], st) and np.array_equal(one_call[2], st) and not st.any()
    s.e.close(); t.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=IDS)
def test_twin_timestamps(spe, model, pname, prec, wide, tol):
    """the ts_us form against the reference in every mode, and against ukfb_predict_timestamps on the twin: every filter its own
    last measurement time, one null, one equal to ts_us[0], one beyond it.  The twin part runs in fp64 and plain fp32: with
    wide_arithmetic the twin narrows its state at every step and the one call does not (test_twin_makes_the_same_predictions),
    and the shadow time of a call cannot be handed to a chained one, so there is no form of the call that computes what the
    twin computes."""
    n = 130
    s, t = pair(spe, model, n, prec, wide)
    last = 1_000_000 + 500 * np.arange(n, dtype=np.int64)
    last[3], last[4], last[5] = 0, 1_070_000, 1_075_000
    ts = np.array([1_070_000, 1_081_000, 1_081_000, 1_093_000, 1_090_000, 1_104_000], dtype=np.int64)
    for x in (s, t):
        x.e.set_last_measurement_time(last)
    got = run(s, ts_us=ts)
    assert np.array_equal(s.e.last_measurement_time(), last), "the forecast moved the engine's last measurement times"
    ref = reference(spe, s, ts_us=ts)
    check_parity(f"{model}/{pname}/ts", s, got, ref, tol, wide)
    assert np.array_equal(got[2], ref[2])
    small_neg = ST_SKIPPED_SMALL_DT | ST_ERR_NEG_DT
    assert got[2][0] == small_neg and got[2][3] == ST_SKIPPED_FIRST_TS | small_neg and got[2][4] == small_neg and got[2][5] == small_neg
    # the filter beyond ts_us[0] and the one without a time are gated at step 0: their record is the start record
    assert np.array_equal(got[0][0, 5], s.e.state()[0][5]) and np.array_equal(got[0][0, 3], s.e.state()[0][3])
    if wide:
        s.e.close(); t.e.close()
        return
    mh, ch = rings_like(t)
    st = np.zeros(n, np.uint32)
    for c in range(STEPS):
        latch(t.e, model, t.host_a[c], t.host_b[c])
        t.e.predict_timestamps(np.full(n, ts[c]))
        st |= t.e.status()
        t.e.history_push_dev(SLOTS, (FIRST + c) % SLOTS, mh, ch)
    t.e.sync()
    report_twin(f"{model}/{pname}/ts", got, sr.window_order(mh.double().cpu().numpy(), FIRST, STEPS),
                sr.window_order(unpack(host(ch), t.e.D), FIRST, STEPS), tol)
    assert np.array_equal(got[2], st)
    assert np.array_equal(t.e.last_measurement_time()[:6], [1_104_000] * 6)   # (the twin's times moved; the forecast's engine kept its own)
    s.e.close(); t.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=IDS)
def test_bitwise_self_consistency(spe, model, pname, prec, wide, tol):
    s, _ = cycled(spe, model, pname)
    e = s.e
    one = run(s)
    # both start pointers NULL = a start at ukfb_device_views (all three modes)
    views = e.device_views()
    dv = run(s, start=(views[0], views[1]))
    assert np.array_equal(one[0], dv[0]) and np.array_equal(one[1], dv[1]) and np.array_equal(one[2], dv[2])
    # no covariance output: the same means
    noc = run(s, cov=False)
    assert np.array_equal(one[0], noc[0]) and noc[1] is None and np.array_equal(one[2], noc[2])
    # the host form is the device form
    hm, hc, hs = e.forecast(dt=s.dt, in_a=sr.window_order(s.in_a.double().cpu().numpy(), FIRST, STEPS),
                            in_b=sr.window_order(s.in_b.double().cpu().numpy(), FIRST, STEPS))
    assert np.array_equal(hm, one[0]) and np.array_equal(hc, one[1]) and np.array_equal(hs, one[2])
    if wide:   # a chained call starts from a record narrowed to fp32: not the chain the one call keeps in fp64
        return
    # one 6-step call = six 1-step calls = 3 + 3, chained through start_*_dev from the slot before (outside the call's window)
    for chunk in (1, 3):
        part = run_chained(s, chunk)
        assert np.array_equal(part[0], one[0]) and np.array_equal(part[1], one[1]) and not part[2].any(), chunk


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_read_only(spe, model):
    """state, initialised flags, status, last measurement times and per-filter noise bit-identical by download around every form
    of the call; the latched inputs through rotation_rate() and -- they have no getter of their own -- through the next
    prediction, which is the one an untouched twin makes"""
    n = 255
    s, twin = pair(spe, model, n, 0, 0, per_filter_noise=True, skip_init=(17,))
    for x in (s, twin):
        x.e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
    before = snapshot(s.e)
    assert same_snapshot(before, snapshot(twin.e)) and len(np.unique(before[5].reshape(n, -1), axis=0)) == n
    ts = 300_000 + 10_000 * np.arange(STEPS, dtype=np.int64)
    forms = [run(s), run(s, rings=False), run(s, cov=False), run(s, ts_us=ts), run(s, start=start_record(s))]
    host = s.e.forecast(dt=s.dt)
    host_ts = s.e.forecast(ts_us=ts, in_a=sr.window_order(s.in_a.cpu().numpy(), FIRST, STEPS),
                           in_b=sr.window_order(s.in_b.cpu().numpy(), FIRST, STEPS), with_cov=False)
    assert same_snapshot(before, snapshot(s.e)), "a forecast call changed the engine"
    assert all(f[2][17] == ST_UNINITIALISED for f in forms) and host[2][17] == ST_UNINITIALISED
    assert np.array_equal(forms[0][0], forms[4][0], equal_nan=True) and np.array_equal(forms[0][1], forms[4][1], equal_nan=True)
    assert np.isnan(forms[0][0][:, 17]).all() and not host[0][:, 17].any()   # nothing written / the host form's zeros
    assert np.array_equal(forms[1][0][:, :17], host[0][:, :17]) and np.array_equal(forms[3][0][:, :17], host_ts[0][:, :17])
    assert not np.array_equal(forms[0][0][:, :17], forms[1][0][:, :17])
    s.e.predict(0.013); twin.e.predict(0.013)
    assert same_snapshot(snapshot(s.e), snapshot(twin.e)), "the prediction after forecasting is not the untouched twin's"
    s.e.close(); twin.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_gated_step_copies_the_previous_steps_bits(spe, model):
    s, _ = cycled(spe, model, "f64")
    dt = s.dt.copy()
    dt[2] = 0.0
    got = run(s, dt=dt)
    ref = reference(spe, s, dt=dt)
    assert (got[2] == ST_SKIPPED_SMALL_DT).all() and (ref[2] == ST_SKIPPED_SMALL_DT).all()
    assert np.array_equal(got[0][2], got[0][1]) and np.array_equal(got[1][2], got[1][1])
    check_parity(f"{model}/f64/gated", s, got, ref, 1e-9, 0)
    # gated at step 0: the start record, bit for bit
    dt[0] = -1.0
    got = run(s, dt=dt)
    mu, cov, _ = s.e.state()
    assert (got[2] == (ST_SKIPPED_SMALL_DT | ST_ERR_NEG_DT)).all()
    assert np.array_equal(got[0][0], mu) and np.array_equal(got[1][0], cov)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failure_and_uninitialised_stay_inside_their_filter(spe, model):
    bad, dead = 13, 22
    s = setup(spe, model, 64, 0, 0, skip_init=(dead,))
    start = start_record(s)
    clean = run(s, start=start)
    D = s.e.D
    poisoned = (start[0], start[1].clone())   # the poison goes into the caller's record, never into the engine
    poisoned[1][bad] = torch.from_numpy(-np.eye(D)[np.tril_indices(D)]).to("cuda", start[1].dtype)
    got = run(s, start=poisoned)
    assert got[2][bad] == ST_ERR_CHOLESKY and got[2][dead] == ST_UNINITIALISED
    others = np.ones(64, bool)
    others[[bad, dead]] = False
    assert (got[2][others] == 0).all() and (clean[2][others] == 0).all()
    # every record of the failing filter is its start record
    smu = start[0][bad].cpu().numpy()
    assert all(np.array_equal(got[0][c, bad], smu) and np.array_equal(got[1][c, bad], -np.eye(D)) for c in range(STEPS))
    # wave-mates: the bits of the run without the poison
    assert np.array_equal(got[0][:, others], clean[0][:, others]) and np.array_equal(got[1][:, others], clean[1][:, others])
    # the uninitialised filter's output slots keep the sentinel
    assert np.isnan(got[0][:, dead]).all() and np.isnan(got[1][:, dead]).all()
    ref = reference(spe, s, start=poisoned)
    assert ref[2][bad] == ST_ERR_CHOLESKY and ref[2][dead] == ST_UNINITIALISED
    check_parity(f"{model}/f64/poisoned", s, got, ref, 1e-9, 0, rows=np.nonzero(others)[0])
    s.e.close()
