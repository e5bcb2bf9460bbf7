"""Inputs of the late sensor-frame sample tests (tests/test_delayed_sensor_reference.py on the CPU,
tests/test_gpu_delayed_sensor.py on the device): the hot history of tests/delayed_reference.py by the NumPy oracle with the
inputs of every step kept (the in-order replay needs them), mounts with a non-trivial qs, points a few metres away, samples
drawn near the recorded state of the sample's OWN step, and the recorder that fills a history ring with history_push_dev
during real cycles.  A helper, not collected.  The recorder is that of tests/test_gpu_delayed.py (no test imports a test: its
statements are repeated here)."""
import numpy as np

from oracle import ukf_numpy as on
import delayed_reference as dr
import sensor_meas_reference as smr
import smoother_reference as sr

ACC_COV = 0.01 * np.eye(3)
STEPS, SLOTS, FIRST = 6, 8, 5
PRECS = [("f64", 0, 0, 1e-9), ("f32", 1, 0, 1e-4), ("f32w", 1, 1, 1e-9 + 2.0 ** -23)]
Q_SAMPLE = 0.05 ** 2 * np.eye(3)


# ------------------------------------------------------------------------------------------------ the hot history on the CPU
def cpu_history(spe, model, n, steps):
    """the recording of the device tests with the NumPy oracle as the filter -> (params, mu [steps, n, S], cov [steps, n, D, D],
    dt, in_a [steps, n, 3], in_b [steps, n, 3], inputs: per step (a, b, model of the in-order cycle, z, Q))"""
    sy = spe.synth
    p = dr.hot_params(sy, model, ACC_COV)
    dt = np.array([dr.HOT_DT * (1.0 + 0.1 * c) for c in range(steps - 1)])
    mu, cov = dr.hot_initial(sy, model, n)
    mus, covs, inputs = [], [], []
    for c in range(steps):
        a, b, mid, z, Q = dr.hot_cycle_inputs(sy, model, n, c, mu)
        if c > 0:
            mu, cov = cpu_cycle(p, mu, cov, inputs[-1][0], inputs[-1][1], dt[c - 1], mid, z, Q)
        inputs.append((a, b, mid, z, Q))
        mus.append(mu); covs.append(cov)
    return p, np.array(mus), np.array(covs), dt, np.array([i[0] for i in inputs]), np.array([i[1] for i in inputs]), inputs


def cpu_cycle(p, mu, cov, a, b, dt, mid, z, Q):
    """one recorded cycle by the NumPy oracle: the prediction with the inputs latched at the previous step, then the update"""
    if p.model == "pose":
        mu, cov, s1 = on.pose_predict(mu, cov, p.R, a, p.acc_cov, dt)
        mu, cov, s2 = on.pose_update(mu, cov, mid, z, Q)
    else:
        mu, cov, s1 = on.orient_predict(mu, cov, p.R, a, b, p.tau_g, p.tau_a, p.earth, dt)
        mu, cov, s2 = on.orient_update(mu, cov, z, Q)
    assert not s1.any() and not s2.any()
    return mu, cov


# ------------------------------------------------------------------------------------------------ mounts, points, samples
def mounts(n, seed=11, lever=1.0):
    """[n, 7]: lever arms of about `lever` metres (0.6 ... 1.2 of it, any direction) and qs = exp(U(-1, 1)^3), far from the identity"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    r = d / np.linalg.norm(d, axis=1, keepdims=True) * lever * rng.uniform(0.6, 1.2, (n, 1))
    return np.concatenate([r, on.so3_exp(rng.uniform(-1.0, 1.0, (n, 3)))], axis=1)


def points(model, n, mu_s, seed=12):
    """[n, 3]: Pose: a landmark / beacon 3 ... 8 m from the filter's position at the sample's step; OrientationState: a nav-frame
    vector of that length"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    away = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3.0, 8.0, (n, 1))
    return (mu_s[:, 0:3] + away) if model == "pose" else away


def rates(n, seed=13):
    """[n, 3]: a rotation rate at the time of the sample, up to 0.6 rad / s"""
    return np.random.default_rng(seed).uniform(-0.6, 0.6, (n, 3))


def cycling_ids(model, n):
    """the engine's own models, cycling: the four rows of a wavefront differ"""
    ids = smr.POSE_IDS if model == "pose" else smr.ORIENT_IDS
    return np.array(ids, dtype=np.int32)[np.arange(n) % len(ids)]


def samples(spe, model, ids, mu_s, mount, point, w=None, seed_offset=41):
    """z [n, 3] of the sensor-frame models `ids` taken near the states mu_s: every component 0.8 ... 1.6 sample sigmas off, so
    that every sample matters; entries beyond m are 0, and so is the sample of an id that is no model of this engine"""
    sy = spe.synth
    n = mu_s.shape[0]
    ids = np.broadcast_to(np.asarray(ids), (n,))
    noise = sy.uniform(sy.SEED_BASE + seed_offset, np.arange(n), [0, 1, 2], -1.0, 1.0)
    noise = np.sign(noise) * (0.04 + 0.04 * np.abs(noise))
    w = np.zeros((n, 3)) if w is None else w
    z = np.zeros((n, 3))
    for mid in np.unique(ids):
        if mid not in (smr.POSE_IDS if model == "pose" else smr.ORIENT_IDS):
            continue   # no model of this engine: the sample stays 0
        i, m = np.nonzero(ids == mid)[0], smr.meas_dim(int(mid))
        z[i, :m] = smr.h(int(mid), mu_s[i], mount[i], point[i], w[i]) + noise[i, :m]
    return z


def state_at_lag(mu_window, mu_n, lag):
    """[n, S]: every filter's recorded state of its own step n - lag (the present for lag 0 and for lags outside the window)"""
    steps, n = mu_window.shape[0], mu_window.shape[1]
    lag = np.broadcast_to(np.asarray(lag), (n,))
    inside = (lag >= 1) & (lag <= steps - 1)
    s = np.where(inside, steps - 1 - lag, 0)
    return np.where(inside[:, None], mu_window[s, np.arange(n)], mu_n)


# ------------------------------------------------------------------------------------------------ the device recorder
class Recording:
    """an engine at the window's last step, its history rings on the device, the inputs of every step"""


def record(spe, model, n, prec, wide, steps=STEPS, slots=SLOTS, first=FIRST, skip_init=(), per_filter_noise=False, **kw):
    """`steps` steps of real cycles on the hot inputs, the filtered state of every step pushed into a ring of `slots` starting at
    slot `first`, the inputs of every step into rings of their own"""
    import torch
    from engine_support import dev, new_engine, tdt
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
    for c in range(steps):
        slot = (first + c) % slots
        mu_now = np.where(live[:, None], e.state(with_cov=False)[0], mu0)
        a, b, mid, z, Q = dr.hot_cycle_inputs(sy, model, n, c, mu_now)
        if c > 0:
            e.cycle(float(r.dt[c - 1]), int(mid), z, Q)
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
    """smoother_reference.Params of a recording's engine, the noise as the engine stores it"""
    e, sy = r.e, spe.synth
    R = np.array([e.process_noise(i) for i in range(r.n)]) if r.per_filter_noise else e.process_noise()
    R = np.asarray(R, dtype=e.dtype).astype(np.float64)
    cfg = e.config()
    kw = dict(min_dt=cfg.min_time_delta, max_dt=cfg.max_time_delta)
    if r.model == "pose":
        return sr.Params("pose", R, acc_cov=np.asarray(2.0 * ACC_COV, dtype=e.dtype).astype(np.float64) / 2.0, **kw)
    return sr.Params("orient", R, tau_g=sy.ORIENT_TAU, tau_a=sy.ORIENT_TAU, earth=on.earth_rotation(sy.ORIENT_LATITUDE), **kw)
