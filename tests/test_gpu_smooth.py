"""Fixed-interval smoothing on the device (ukfb_history_push_dev / ukfb_smooth_dev / ukfb_smooth, include/ukf_batch.h).

The history is recorded with history_push_dev during real cycles (Pose: the acceleration branch with every fifth filter on a NaN
acceleration row, POS3 updates; OrientationState: its body-velocity update; inputs from synth) into a ring of 8 slots that the
window of 6 steps wraps (first slot 5).  The reference is tests/smoother_reference.py (pinned by
tests/test_smoother_reference.py) run on the history AS DOWNLOADED, so that storage rounding of the inputs is out of the
comparison.  Parity bound: |x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64) / 1e-4 (fp32) / 1e-9 + 2^-23 (fp32 engines with
wide_arithmetic, against the reference's outputs rounded to fp32).  The maxima measured on an MI355X are in
profiles/smoother_parity.txt.

Every parity comparison also makes the SCALED one (tests/feature_scaled_parity.py): every step of the smoothed window, whitened by the
reference's own sigmas and held block by block -- fp64 1e-9; wide_arithmetic 2 u v + 1e-9 against the float64 reference on the
inputs as stored (the kernel narrows each stored output once); plain fp32 max(M_feat d_32, 20 u v), d_32 the distance of the
all-float32 evaluation of the same call (tests/feature_f32.py) from its float64 evaluation on the same batch.  It prints one
SCALED line: the largest fraction of a bound and the block it belongs to.  The chain is never narrowed
below the arithmetic type between steps (CSM / CSP of ukf_smooth.hpp), so every step's record is one rounding from the chain:
c = 1 for every step of the window, whatever its length (6 steps, and 12 steps in test_parity_twelve_steps).
"""
import os

import numpy as np
import pytest
import torch

import feature_f32 as ff
import feature_scaled_parity as fsp
import smoother_reference as sr
from engine_support import host, new_engine, same_snapshot, scaled, snapshot, tdt, unpack

pytestmark = pytest.mark.gpu

N = 1022   # not a multiple of four: the last workgroup holds two filters
STEPS, SLOTS, FIRST = 6, 8, 5
PRECS = [("f64", 0, 0, 1e-9), ("f32", 1, 0, 1e-4), ("f32w", 1, 1, 1e-9 + 2.0 ** -23)]
ACC_COV = 0.01 * np.eye(3)
ST_SKIPPED_SMALL_DT, ST_ERR_CHOLESKY, ST_UNINITIALISED = 1 << 1, 1 << 5, 1 << 7


class Recording:
    """an engine, its history rings on the device, the inputs and states of every step as the host saw them"""


def record(spe, model, n, prec, wide, steps=STEPS, slots=SLOTS, first=FIRST, skip_init=(), keep_states=False,
           per_filter_noise=False, **kw):
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
    r = Recording()
    r.e, r.model, r.n, r.steps, r.slots, r.first = e, model, n, steps, slots, first
    r.mu_hist = torch.zeros((slots, n, e.S), dtype=tdt(e), device="cuda")
    r.cov_hist = torch.zeros((slots, n, e.PK), dtype=tdt(e), device="cuda")
    r.in_a = torch.zeros((slots, n, 3), dtype=tdt(e), device="cuda")
    r.in_b = torch.zeros((slots, n, 3), dtype=tdt(e), device="cuda")
    r.dt = np.array([0.01 * (1.0 + 0.1 * c) for c in range(steps - 1)])
    r.states = []
    r.live = live
    r.per_filter_noise = per_filter_noise
    for c in range(steps):
        slot = (first + c) % slots
        mu_now = e.state(with_cov=False)[0]
        if model == "pose":
            acc, z, Q = sy.pose_cycle_inputs(n, c, mu_now[:, :3])
            acc[::5] = np.nan   # the constant-velocity branch
            a, b = acc, np.zeros((n, 3))
        else:
            gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu_now[:, 0:4])
            a, b = acc, gyro
        if c > 0:
            e.cycle(float(r.dt[c - 1]), spe.MEAS_POS3 if model == "pose" else spe.MEAS_ORIENT_BODYVEL3, z, Q)
        e.history_push_dev(slots, slot, r.mu_hist, r.cov_hist)
        if keep_states:
            r.states.append(e.state())
        # the inputs of the prediction c -> c + 1: latched now, and into the ring at step c's slot
        if model == "pose":
            e.set_acceleration(a, ACC_COV)
        else:
            e.set_orient_inputs(b, a)
        r.in_a[slot] = torch.from_numpy(a).to("cuda", tdt(e))
        r.in_b[slot] = torch.from_numpy(b).to("cuda", tdt(e))
    # what the engine's own latches hold from here on, as stored
    r.latch_a, r.latch_b = a.astype(e.dtype).astype(np.float64), b.astype(e.dtype).astype(np.float64)
    return r


def reference(spe, r, mu_hist=None, cov_hist=None, dt=None, steps=None, first=None, rings=True):
    e, sy = r.e, spe.synth
    steps = r.steps if steps is None else steps
    first = r.first if first is None else first
    mu = sr.window_order((r.mu_hist if mu_hist is None else mu_hist).double().cpu().numpy(), first, steps)
    cov = sr.window_order(unpack(host(r.cov_hist if cov_hist is None else cov_hist), e.D), first, steps)
    a = sr.window_order(r.in_a.double().cpu().numpy(), first, steps)
    b = sr.window_order(r.in_b.double().cpu().numpy(), first, steps)
    if not rings:   # the engine's latched inputs serve every step
        a, b = r.latch_a, r.latch_b
    R = np.array([e.process_noise(i) for i in range(r.n)]) if r.per_filter_noise else e.process_noise()
    R = np.asarray(R, dtype=e.dtype).astype(np.float64)
    dt = (r.dt if dt is None else dt)[:steps - 1]
    if r.model == "pose":
        p = sr.Params("pose", R, acc_cov=np.asarray(2.0 * ACC_COV, dtype=e.dtype).astype(np.float64) / 2.0)
        return Reference(sr.smooth(p, mu, cov, dt, in_a=a, initialised=r.live), (p, mu, cov, dt, a, None))
    from oracle import ukf_numpy as on
    p = sr.Params("orient", R, tau_g=sy.ORIENT_TAU, tau_a=sy.ORIENT_TAU, earth=on.earth_rotation(sy.ORIENT_LATITUDE))
    return Reference(sr.smooth(p, mu, cov, dt, in_a=a, in_b=b, initialised=r.live), (p, mu, cov, dt, a, b))


class Reference(tuple):
    """the result of smoother_reference.smooth, and in .call what it was called with (for the fp32 evaluation of the same call)"""

    def __new__(cls, result, call):
        self = super().__new__(cls, result)
        self.call = call
        return self


def run(r, dt=None, steps=None, first=None, mu_hist=None, cov_hist=None, in_place=False, cov=True, rings=True):
    """-> (mu_s [steps, n, S], cov_s [steps, n, D, D] or None, status [n]) in window order"""
    e = r.e
    steps = r.steps if steps is None else steps
    first = r.first if first is None else first
    mh = r.mu_hist if mu_hist is None else mu_hist
    ch = r.cov_hist if cov_hist is None else cov_hist
    if in_place:
        mh, ch = mh.clone(), ch.clone()
        mo, co = mh, ch
    else:
        mo = torch.full_like(mh, float("nan"))
        co = torch.full_like(ch, float("nan")) if cov else False
    st = torch.full((r.n,), -1, dtype=torch.int32, device="cuda")
    e.smooth_dev((r.dt if dt is None else dt)[:steps - 1], r.slots, first, mh, ch, mo, co, st,
                 in_a_dev=r.in_a if rings else None, in_b_dev=r.in_b if rings else None)
    torch.cuda.synchronize()
    mu_s = sr.window_order(mo.double().cpu().numpy(), first, steps)
    cov_s = sr.window_order(unpack(host(co), e.D), first, steps) if co is not False else None
    return mu_s, cov_s, st.cpu().numpy().astype(np.uint32), (mo, co)


def check_parity(name, r, got, ref, tol, wide, rows=slice(None), unscaled=()):
    """the file's bound, then the scaled check of every step of the window (tests/feature_scaled_parity.py).  unscaled:
    (step, filter) records whose reference covariance is no covariance (a poisoned record is passed through as it is): they
    have no sigma to be measured in and keep the file's bound alone"""
    mu_s, cov_s, _, _ = got
    mu_r, cov_r = ref[0], ref[1]
    if wide:   # the engine stores fp32
        mu_r, cov_r = mu_r.astype(np.float32).astype(np.float64), cov_r.astype(np.float32).astype(np.float64)
    em, ec = scaled(mu_s[:, rows], mu_r[:, rows]), scaled(cov_s[:, rows], cov_r[:, rows])
    print(f"PARITY {name} n={r.n} steps={mu_s.shape[0]} max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e} tol={tol:.3e}")
    assert em <= tol and ec <= tol, (name, em, ec, tol)
    mode = "wide" if wide else ("f64" if r.e.dtype == np.float64 else "f32")
    p, mu, cov, dt, a, b = ref.call
    pick = np.zeros(mu_s.shape[:2], bool)
    pick[:, rows] = True
    for c, f in unscaled:
        pick[c, f] = False

    def f32():
        return tuple(ff.smooth(p, mu, cov, dt, a, b, prec=q) for q in ("f32", "f64"))
    fsp.judge_state("smooth/" + name, r.model, mode, mu_s, cov_s, ref[0], ref[1], f32=f32, rows=pick.reshape(-1))


_CACHE = {}


def recorded(spe, model, pname):
    key = (model, pname)
    if key not in _CACHE:
        _, prec, wide, _ = [p for p in PRECS if p[0] == pname][0]
        r = record(spe, model, N, prec, wide)
        _CACHE[key] = (r, reference(spe, r))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS)
def test_parity(spe, model, pname, prec, wide, tol):
    r, ref = recorded(spe, model, pname)
    got = run(r)
    assert (ref[2] == 0).all()
    assert (got[2] == 0).all(), np.unique(got[2])
    check_parity(f"{model}/{pname}", r, got, ref, tol, wide)
    # the last step is the filtered record, bit for bit
    last = (FIRST + STEPS - 1) % SLOTS
    assert torch.equal(got[3][0][last], r.mu_hist[last]) and torch.equal(got[3][1][last], r.cov_hist[last])


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_parity_twelve_steps(spe, model, pname, prec, wide, tol):
    """12 steps in a ring of 16 that the window wraps (first slot 9), 203 filters, one launch: the backward chain passes eleven
    steps through the small blocks (gyro bias, accelerometer bias, angular velocity), where the 6-step window passes five"""
    steps, slots, first = 12, 16, 9
    r = record(spe, model, 203, prec, wide, steps=steps, slots=slots, first=first)
    got, ref = run(r), reference(spe, r)
    assert (ref[2] == 0).all()
    assert (got[2] == 0).all(), np.unique(got[2])
    assert got[0].shape[0] == steps
    check_parity(f"{model}/{pname}/12-steps", r, got, ref, tol, wide)
    last = (first + steps - 1) % slots
    assert torch.equal(got[3][0][last], r.mu_hist[last]) and torch.equal(got[3][1][last], r.cov_hist[last])
    r.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_history_push_is_the_state_bit_for_bit(spe, model):
    r = record(spe, model, 255, 0, 0, keep_states=True)
    mu = sr.window_order(r.mu_hist.cpu().numpy(), FIRST, STEPS)
    cov = sr.window_order(unpack(host(r.cov_hist), r.e.D), FIRST, STEPS)
    for c, (m, C, _) in enumerate(r.states):
        assert np.array_equal(mu[c], m) and np.array_equal(cov[c], C), c


def test_history_push_follows_a_split_launch_without_sync(spe):
    """16 384 filters on an engine that owns its stream: launches run as two halves on two internal streams"""
    sy, n = spe.synth, 16384
    e = spe.BatchPoseUKF(n, precision=spe.F32, stream="private")
    mu0, cov0 = sy.pose_initial(n)
    e.initialize(mu0, cov0)
    acc, z, Q = sy.pose_cycle_inputs(n, 0, mu0[:, :3])
    e.set_acceleration(acc, ACC_COV)
    zd = torch.from_numpy(z).to("cuda", torch.float32)
    Qd = torch.from_numpy(Q.reshape(n, 9)).to("cuda", torch.float32)
    mh = torch.zeros((2, n, e.S), dtype=torch.float32, device="cuda")
    ch = torch.zeros((2, n, e.PK), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for c in range(3):
        e.cycle_dev(0.01, spe.MEAS_POS3, zd, Qd)
        e.history_push_dev(2, c % 2, mh, ch)   # no ukfb_sync in between
    e.sync()
    m, C, _ = e.state()
    # the launches above were split: the conditions of split_launch (ukf_host.hpp; tests/cpp/smooth_host.cpp pins that this
    # shape meets them) -- a direct launch of the tuned kernel on an engine that owns its stream, with split_streams on
    assert e.stream_kind == "private" and e.config().split_streams == 1 and e.config().lanes_per_filter in (0, 16)
    assert "ukf_kernel16" in e.last_launch_info()["kernel"] and e.last_launch_info()["grid"] == n // 4
    assert not os.environ.get("UKFB_SPLIT_MAX")
    assert np.array_equal(mh[0].double().cpu().numpy(), m) and np.array_equal(unpack(host(ch[0]), e.D), C)
    assert not np.array_equal(mh[1].double().cpu().numpy(), m)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_read_only_in_place_and_no_covariance(spe, model):
    """state, status, last measurement times and per-filter noise bit-identical by download; the latched inputs through
    rotation_rate() and -- they have no getter of their own -- through the next prediction, which is the one an untouched twin
    makes (the twin saw the same recording and no smoother call)"""
    n = 255
    r = record(spe, model, n, 0, 0, per_filter_noise=True)
    twin = record(spe, model, n, 0, 0, per_filter_noise=True)
    for x in (r, twin):
        x.e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
    before = snapshot(r.e)
    assert same_snapshot(before, snapshot(twin.e)) and len(np.unique(before[5].reshape(n, -1), axis=0)) == n
    assert torch.equal(r.mu_hist, twin.mu_hist) and torch.equal(r.cov_hist, twin.cov_hist)
    out = run(r)
    inp = run(r, in_place=True)
    noc = run(r, cov=False)
    lat = run(r, rings=False)
    mu = sr.window_order(r.mu_hist.cpu().numpy(), FIRST, STEPS)
    host_form = r.e.smooth(r.dt, mu, sr.window_order(unpack(host(r.cov_hist), r.e.D), FIRST, STEPS),
                           in_a=sr.window_order(r.in_a.cpu().numpy(), FIRST, STEPS), in_b=sr.window_order(r.in_b.cpu().numpy(), FIRST, STEPS))
    assert same_snapshot(before, snapshot(r.e)), "a smoother call changed the engine"
    r.e.predict(0.013); twin.e.predict(0.013)
    assert same_snapshot(snapshot(r.e), snapshot(twin.e)), "the prediction after smoothing is not the untouched twin's"
    assert np.array_equal(out[0], inp[0]) and np.array_equal(out[1], inp[1]) and np.array_equal(out[2], inp[2])
    assert np.array_equal(out[0], noc[0]) and noc[1] is None
    assert np.array_equal(out[0], host_form[0]) and np.array_equal(out[1], host_form[1])
    assert (lat[2] == 0).all() and not np.array_equal(lat[0], out[0])
    r.e.close(); twin.e.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS[:2], ids=[p[0] for p in PRECS[:2]])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_parity_latched_inputs_and_per_filter_noise(spe, model, pname, prec, wide, tol):
    """the two paths the base recording does not take: NULL input rings (the engine's latches serve every step) and a process
    noise per filter (strided Rn and, Pose, Racc)"""
    r = record(spe, model, 254, prec, wide, per_filter_noise=True)
    for rings in (True, False):
        got, ref = run(r, rings=rings), reference(spe, r, rings=rings)
        assert (got[2] == 0).all() and (ref[2] == 0).all()
        check_parity(f"{model}/{pname}/per-filter-noise/{'rings' if rings else 'latches'}", r, got, ref, tol, wide)
    r.e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_chain_residency_one_call_equals_chained_calls(spe, model):
    r, _ = recorded(spe, model, "f64")
    one = run(r)
    mh, ch = r.mu_hist.clone(), r.cov_hist.clone()
    for c in range(STEPS - 2, -1, -1):   # five calls over 2 steps, each fed by the one above, in place
        st = torch.zeros(r.n, dtype=torch.int32, device="cuda")
        r.e.smooth_dev(r.dt[c:c + 1], SLOTS, (FIRST + c) % SLOTS, mh, ch, None, None, st, in_a_dev=r.in_a, in_b_dev=r.in_b)
        assert int(st.abs().max()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(sr.window_order(mh.cpu().numpy(), FIRST, STEPS), one[0])
    assert np.array_equal(sr.window_order(unpack(host(ch), r.e.D), FIRST, STEPS), one[1])


def test_chunking_two_launches(spe):
    """35 steps in a ring of 40: 34 backward steps = two launches (32 + 2)"""
    steps, slots, first = 35, 40, 9
    r = record(spe, "pose", 64, 0, 0, steps=steps, slots=slots, first=first)
    whole = run(r)
    ref = reference(spe, r)
    check_parity("pose/f64/35-steps", r, whole, ref, 1e-9, 0)
    assert (whole[2] == 0).all()
    # the same by hand: steps 31 ... 34 first, then steps 0 ... 31 fed by it, in place
    mh, ch = r.mu_hist.clone(), r.cov_hist.clone()
    r.e.smooth_dev(r.dt[31:34], slots, (first + 31) % slots, mh, ch, in_a_dev=r.in_a, in_b_dev=r.in_b)
    r.e.smooth_dev(r.dt[0:31], slots, first, mh, ch, in_a_dev=r.in_a, in_b_dev=r.in_b)
    torch.cuda.synchronize()
    assert np.array_equal(sr.window_order(mh.cpu().numpy(), first, steps), whole[0])
    assert np.array_equal(sr.window_order(unpack(host(ch), r.e.D), first, steps), whole[1])
    # no covariance output: the chain's covariance crosses the launch boundary through the engine's workspace -- the same means
    noc = run(r, cov=False)
    assert np.array_equal(noc[0], whole[0]) and noc[1] is None and (noc[2] == 0).all()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_gated_step_copies_the_next_steps_bits(spe, model):
    r, _ = recorded(spe, model, "f64")
    dt = r.dt.copy()
    dt[2] = 0.0
    got = run(r, dt=dt)
    ref = reference(spe, r, dt=dt)
    assert (got[2] == ST_SKIPPED_SMALL_DT).all() and (ref[2] == ST_SKIPPED_SMALL_DT).all()
    assert np.array_equal(got[0][2], got[0][3]) and np.array_equal(got[1][2], got[1][3])
    check_parity(f"{model}/f64/gated", r, got, ref, 1e-9, 0)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failure_and_uninitialised_stay_inside_their_filter(spe, model):
    bad, dead, step = 13, 22, 3
    r = record(spe, model, 64, 0, 0, skip_init=(dead,))
    clean = run(r)
    ch = r.cov_hist.clone()   # the poison goes into the caller's ring, never into the engine
    D = r.e.D
    ind = -np.eye(D)[np.tril_indices(D)]
    ch[(FIRST + step) % SLOTS, bad] = torch.from_numpy(ind).to("cuda", ch.dtype)
    got = run(r, cov_hist=ch)
    ref = reference(spe, r, cov_hist=ch)
    assert got[2][bad] == ST_ERR_CHOLESKY and ref[2][bad] == ST_ERR_CHOLESKY
    assert got[2][dead] == ST_UNINITIALISED
    others = np.ones(64, bool)
    others[[bad, dead]] = False
    assert (got[2][others] == 0).all()
    # the failing step is the filtered record, the steps below it follow the reference (which applies the same rule)
    hist_mu = sr.window_order(r.mu_hist.cpu().numpy(), FIRST, STEPS)
    assert np.array_equal(got[0][step, bad], hist_mu[step, bad])
    assert np.array_equal(got[1][step, bad], -np.eye(D))
    check_parity(f"{model}/f64/poisoned", r, got, ref, 1e-9, 0, rows=np.nonzero(others | (np.arange(64) == bad))[0],
                 unscaled=[(c, bad) for c in range(step + 1)])
    # wave-mates: the bits of the run without the poison
    assert np.array_equal(got[0][:, others], clean[0][:, others]) and np.array_equal(got[1][:, others], clean[1][:, others])
    # the uninitialised filter's output slots keep the sentinel
    assert np.isnan(got[0][:, dead]).all() and np.isnan(got[1][:, dead]).all()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS)
def test_host_array_form(spe, pname, prec, wide, tol):
    r, _ = recorded(spe, "pose", pname)
    dev = run(r)
    mu = sr.window_order(r.mu_hist.double().cpu().numpy(), FIRST, STEPS)
    cov = sr.window_order(unpack(host(r.cov_hist), r.e.D), FIRST, STEPS)
    a = sr.window_order(r.in_a.double().cpu().numpy(), FIRST, STEPS)
    mu_s, cov_s, st = r.e.smooth(r.dt, mu, cov, in_a=a)
    assert (st == 0).all()
    assert np.array_equal(mu_s, dev[0]) and np.array_equal(cov_s, dev[1])   # the same records in, the same kernel
