"""Every launch path against the CPU oracle with each block of the state held to its own sigma (tests/scaled_parity.py).

The other parity files bound max |x - ref| over all entries by 1e-9 (fp64) / 1e-4 (fp32).  The states are not of one scale:
an fp32 OrientationState kernel could zero the gyro-bias covariance block (variance 1e-6) or be 100 % off in the accelerometer-bias
and gravity blocks and pass them all.  Here the distance is taken in the reference's whitened metric, per mean block and per pair
of covariance blocks, every filter counted, against

    fp64 engine   1e-9
    wide fp32     2 c u v + 1e-9 from the fp64 oracle chain rounded to fp32 at each of its c commits
    fp32 engine   max(M d_o32, 20 u v), d_o32 the float oracle's own distance, M from the CPU alone (profiles/scaled_parity.txt)

(u = 2^-24, v = the block's largest magnitude / sigma).  A multi-cycle launch of the wide engine narrows its state once, at the
end of the launch (tests/test_gpu_wide_arithmetic.py), the reference at every cycle: c + 1 roundings between them, within 2 c.
No bound in this file comes from GPU output.  n = 203 everywhere (a ragged tail at 4, 2 and 1 filters per wavefront) but for one
launch of 16 387 filters, the smallest size at which model buckets and split streams engage.  Every case asserts its kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scaled_parity as sp  # noqa: E402

pytestmark = pytest.mark.gpu

N = 203
DT = 0.01
MODELS = ("pose", "orient")
TAG = {"f64": "f64", "f32": "f32", "wide": "f32-wide"}
_CASES = {}


def _case(spe, model, mode, n=N, noise="default"):
    """the input sets are built once and shared (nothing modifies them)"""
    key = (model, mode, n, noise)
    if key not in _CASES:
        _CASES[key] = sp.Case(spe, model, mode, n, noise)
    return _CASES[key]


def _engine(c, lanes=0, **kw):
    spe, s = c.spe, c.spe.synth
    prec = spe.F64 if c.mode == "f64" else spe.F32
    if c.mode == "wide":
        kw["wide_arithmetic"] = 1
    if lanes:
        kw["lanes_per_filter"] = lanes
    if c.model == "pose":
        e = spe.BatchPoseUKF(c.n, precision=prec, **kw)
    else:
        e = spe.BatchOrientationUKF(c.n, s.ORIENT_TAU, s.ORIENT_TAU, s.ORIENT_LATITUDE, precision=prec, **kw)
    if c.R.ndim == 3:
        e.set_process_noise(c.R, first=0)
    else:
        e.set_process_noise(c.R)
    e.initialize(c.mu, c.cov)
    if c.model == "pose":
        e.set_acceleration(c.acc, c.acc_cov)
    else:
        e.set_orient_inputs(c.gyro, c.acc)
    return e


def _dev(c, x):
    import torch
    x = np.asarray(x)
    t = torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1))).to("cuda", torch.float64 if c.mode == "f64" else torch.float32)
    torch.cuda.synchronize()
    return t


def _ring(c, xs):
    import torch
    t = torch.stack([_dev(c, x) for x in xs]).contiguous()
    torch.cuda.synchronize()
    return t


def _kernel(e, c, shape, lanes=16):
    name = e.last_launch_info()["kernel"]
    want = (f"ukf_kernel16<{TAG[c.mode]},{c.model},{shape}>" if lanes == 16
            else f"ukf_kernel<{TAG[c.mode]},{c.model},G{lanes},{shape.replace('-plain', '')}>")
    assert name == want, (name, want)


def _judge(e, c, ops, what, rows=None):
    m, cv, init = e.state()
    st = e.status()
    assert init.all()
    if rows is not None:
        m, cv, st = m[rows], cv[rows], st[rows]
    return sp.judge(c, ops, m, cv, st, what, rows=rows)


def _general(fn):
    os.environ["UKFB_NO_PLAIN_KERNEL"] = "1"
    try:
        return fn()
    finally:
        os.environ.pop("UKFB_NO_PLAIN_KERNEL", None)


# (mode, lanes per filter, general instantiation).  The plain / general split exists on the tuned layout (16 lanes) only: the
# one-wavefront-per-filter layouts (32, 64 lanes; fp32 builds) have ONE instantiation per launch shape, which ignores
# UKFB_NO_PLAIN_KERNEL and is named without a suffix -- no general case is left out for them.
LAYOUTS = [(m, 16, g) for m in sp.MODES for g in (0, 1)] + [("f32", 32, 0), ("f32", 64, 0)]


# ------------------------------------------------------------------------------------------------------ predict
@pytest.mark.parametrize("mode,lanes,general", LAYOUTS)
@pytest.mark.parametrize("model", MODELS)
def test_predict(spe, model, mode, lanes, general):
    """Pose: acceleration and constant-velocity branches inside each wavefront, a dense acceleration covariance; OrientationState:
    orient_process_noise(), 1e-12 ... 1e-4.  On 16 lanes once as the plain and once as the general instantiation; on 32 and 64
    lanes the layout's single instantiation (there is no plain / general split to run twice)"""
    c = _case(spe, model, mode)
    e = _engine(c, lanes)
    if general:
        _general(lambda: e.predict(DT))
    else:
        e.predict(DT)
    _kernel(e, c, "predict" if general else "predict-plain", lanes)
    _judge(e, c, [("predict", DT), ("commit",)], "predict")
    e.close()


# ------------------------------------------------------------------------------------------------------ update
@pytest.mark.parametrize("mode", sp.MODES)
@pytest.mark.parametrize("meas", list(range(10)))
def test_update_every_model(spe, meas, mode):
    """Pose models 0 ... 8 and OrientationState BODYVEL3, per-filter Q"""
    model = "orient" if meas == spe.MEAS_ORIENT_BODYVEL3 else "pose"
    c = _case(spe, model, mode)
    z = c.z_for(meas)
    e = _engine(c)
    e.update(meas, z, c.Q)
    full3 = meas in (spe.MEAS_POS3, spe.MEAS_VEL3, spe.MEAS_ANGVEL3, spe.MEAS_ORIENT_BODYVEL3)
    _kernel(e, c, "update-plain" if full3 else "update-streams")
    _judge(e, c, [("update", meas, z, c.Q), ("commit",)], f"update model {meas}")
    e.close()


@pytest.mark.parametrize("mode", sp.MODES)
@pytest.mark.parametrize("model", MODELS)
def test_update_uniform_q(spe, model, mode):
    c = _case(spe, model, mode)
    Q1 = c.r(np.array([[0.004, 0.001, 0.0], [0.001, 0.003, -0.0005], [0.0, -0.0005, 0.002]]))
    Qn = np.broadcast_to(Q1, (c.n, 3, 3)).copy()
    e = _engine(c)
    e.update_uniform_q(c.full3, c.z, Q1)
    _kernel(e, c, "update-plain")
    _judge(e, c, [("update", c.full3, c.z, Qn), ("commit",)], "update, uniform Q")
    e.close()


@pytest.mark.parametrize("mode", sp.MODES)
@pytest.mark.parametrize("model", MODELS)
def test_update_per_filter_models_inactive_unchanged(spe, model, mode):
    """per-filter model ids (OrientationState: an activity mask), 25 % of the filters without a sample: those keep their bits"""
    c = _case(spe, model, mode)
    models = spe.synth.pose_mixed_models(c.n, 0)
    off = models < 0
    assert 0.15 * c.n < off.sum() < 0.35 * c.n
    e = _engine(c)
    if model == "pose":
        z = c.z_for(models)
        e.update(models, z, c.Q)
        _kernel(e, c, "update-streams")
    else:
        models = np.where(off, -1, spe.MEAS_ORIENT_BODYVEL3).astype(np.int32)
        z = c.z
        e.update(spe.MEAS_ORIENT_BODYVEL3, z, c.Q, active=(~off).astype(np.uint8))
        _kernel(e, c, "update")
    m, cv, _ = e.state()
    assert np.array_equal(m[off], c.mu[off]) and np.array_equal(cv[off], c.cov[off])
    assert (e.status()[off] == spe.ST_INACTIVE).all()
    _judge(e, c, [("update", models, z, c.Q), ("commit",)], "update, per-filter models")
    e.close()


# ------------------------------------------------------------------------------------------------------ fused cycle
@pytest.mark.parametrize("form", ["plain", "plain-full-check", "streams", "timestamps", "uniform-q", "per-filter-noise"])
@pytest.mark.parametrize("mode", sp.MODES)
@pytest.mark.parametrize("model", MODELS)
def test_fused_cycle(spe, model, mode, form):
    import torch
    c = _case(spe, model, mode, noise="per_filter" if form == "per-filter-noise" else "default")
    e = _engine(c, **({"full_update_check": 1} if form == "plain-full-check" else {}))
    assert e.config().full_update_check == (1 if form == "plain-full-check" else 0)
    z, Q, models, dt = c.z, c.Q, c.full3, DT
    if form in ("plain", "plain-full-check", "per-filter-noise"):
        e.cycle_dev(DT, c.full3, _dev(c, z), _dev(c, Q))
        _kernel(e, c, "cycle-plain")
    elif form == "streams":
        if model == "pose":
            models = spe.synth.pose_mixed_models(c.n, 0)
            z = c.z_for(models)
        else:
            models = np.where(np.arange(c.n) % 4 == 1, -1, c.full3).astype(np.int32)
        e.cycle_dev(DT, 0, _dev(c, z), _dev(c, Q), meas_model_dev=torch.from_numpy(models).to("cuda"))
        _kernel(e, c, "cycle-streams")
    elif form == "timestamps":
        t0 = 5_000_000
        ts = t0 + 10_000 + 37 * (np.arange(c.n, dtype=np.int64) % 97)
        e.set_last_measurement_time(np.full(c.n, t0, dtype=np.int64))
        e.cycle_timestamps(ts, np.full(c.n, c.full3, dtype=np.int32), z, Q)
        _kernel(e, c, "cycle")
        dt = (ts - t0) / 1e6
    else:
        Q1 = c.r(np.array([[0.004, 0.001, 0.0], [0.001, 0.003, -0.0005], [0.0, -0.0005, 0.002]]))
        Q = np.broadcast_to(Q1, (c.n, 3, 3)).copy()
        e.cycle_uniform_q(DT, c.full3, z, Q1)
        _kernel(e, c, "cycle-plain")
    _judge(e, c, [("predict", dt), ("update", models, z, Q), ("commit",)], f"cycle, {form}")
    e.close()


# ------------------------------------------------------------------------------------------------------ three-cycle chains
def _three(c):
    zs = [c.z_for(c.full3, k) for k in range(3)]
    return zs, [c.Q] * 3


@pytest.mark.parametrize("form", ["multi", "schedule"])
@pytest.mark.parametrize("mode", sp.MODES)
@pytest.mark.parametrize("model", MODELS)
def test_three_cycle_launch(spe, model, mode, form):
    """three cycles in one launch: the cross-covariances between the small and the large blocks fill in"""
    c = _case(spe, model, mode)
    zs, Qs = _three(c)
    z_r, Q_r = _ring(c, zs), _ring(c, Qs)
    e = _engine(c)
    ops = []
    if form == "multi":
        e.cycle_multi_dev(3, DT, c.full3, z_r, Q_r, 3, 0)
        _kernel(e, c, "multicycle-plain")
        for k in range(3):
            ops += [("predict", DT), ("update", c.full3, zs[k], Qs[k]), ("commit",)]
    else:
        dts = [DT, 2 * DT, DT]
        e.cycle_schedule_dev(dts, [c.full3, -1, c.full3], z_r, Q_r, 3, 0)
        _kernel(e, c, "multicycle")
        ops = [("predict", dts[0]), ("update", c.full3, zs[0], Qs[0]), ("commit",), ("predict", dts[1]), ("commit",),
               ("predict", dts[2]), ("update", c.full3, zs[2], Qs[2]), ("commit",)]
    _judge(e, c, ops, f"three cycles, {form}")
    e.close()


@pytest.mark.parametrize("mode", sp.MODES)
def test_three_cycle_mixed_models(spe, mode):
    import torch
    c = _case(spe, "pose", mode)
    mods = [spe.synth.pose_mixed_models(c.n, k) for k in range(3)]
    zs = [c.z_for(m, k) for k, m in enumerate(mods)]
    e = _engine(c)
    m_r = torch.from_numpy(np.stack(mods).astype(np.int32)).cuda().contiguous()
    e.cycle_multi_mixed_dev(3, DT, m_r, _ring(c, zs), _ring(c, [c.Q] * 3), 3, 0)
    _kernel(e, c, "multicycle")
    ops = []
    for k in range(3):
        ops += [("predict", DT), ("update", mods[k], zs[k], c.Q), ("commit",)]
    _judge(e, c, ops, "three cycles, per-filter models")
    e.close()


@pytest.mark.parametrize("mode", sp.MODES)
@pytest.mark.parametrize("model", MODELS)
def test_three_event_rounds(spe, oracle, model, mode):
    """one stream of three samples per filter, in arbitrary order: three rounds of indirect launches"""
    c = _case(spe, model, mode)
    n = c.n
    zs, Qs = _three(c)
    t0 = 5_000_000
    ts = [t0 + 10_000 * (k + 1) + 37 * (np.arange(n, dtype=np.int64) % 97) * (k + 1) for k in range(3)]
    perm = np.random.default_rng(5).permutation(3 * n)
    cat = lambda xs: np.concatenate(xs)[perm]                                     # noqa: E731
    e = _engine(c)
    e.set_last_measurement_time(np.full(n, t0, dtype=np.int64))
    st_or, rounds = e.process_events(cat([np.arange(n)] * 3), cat(ts), np.full(3 * n, c.full3, dtype=np.int32), cat(zs), cat(Qs))
    assert rounds == 3 and st_or == 0
    assert e.last_launch_info()["kernel"].startswith(f"ukf_kernel16<{TAG[mode]},{model},cycle")
    ops, last = [], np.full(n, t0, dtype=np.int64)
    for k in range(3):
        last, dts, gs = oracle.gate_timestamps(ts[k], last)
        assert (gs == 0).all()
        ops += [("predict", dts), ("update", c.full3, zs[k], Qs[k]), ("commit",)]
    _judge(e, c, ops, "three event rounds")
    e.close()


# ------------------------------------------------------------------------------------------------------ buckets and split streams
@pytest.mark.parametrize("mode", sp.MODES)
def test_bucketed_split_launch(spe, mode):
    """16 387 filters with per-filter model ids on an engine that owns its stream: grouped by update class (one launch
    over the grouped list; split_streams is on, as for every launch of such an engine at this size).  The oracle runs on a strided sample of 512 filters and the first and last 8 of each half."""
    import torch
    n = 16_387
    c = _case(spe, "pose", mode, n=n)
    models = spe.synth.pose_mixed_models(n, 0)
    z = c.z_for(models)
    e = _engine(c, stream="private")
    assert e.stream_kind == "private" and e.config().split_streams == 1 and e.config().bucket_models == 1
    m_t, z_t, Q_t = torch.from_numpy(models).to("cuda"), _dev(c, z), _dev(c, c.Q)
    torch.cuda.synchronize()                      # (the engine's own stream does not wait for torch's)
    e.cycle_dev(DT, 0, z_t, Q_t, meas_model_dev=m_t)
    e.sync()
    _kernel(e, c, "cycle-bucketed-streams")
    h = (n // 2 + 3) // 4 * 4
    rows = np.unique(np.concatenate([np.arange(0, n, n // 512)[:512], np.arange(8), np.arange(h - 8, h + 8), np.arange(n - 8, n)]))
    _judge(e, c, [("predict", DT), ("update", models, z, c.Q), ("commit",)], "bucketed split cycle", rows=rows)
    e.close()
