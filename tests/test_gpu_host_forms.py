"""Every host-array form of the C ABI against its device form, bit for bit, at shapes where a wrong element count shows.

The 17 host-array forms (ukfb_innovation ... ukfb_update_delayed, include/ukf_batch.h) stage their `double*` / `int32_t*` host
arrays on the device in the engine's precision, call the `_dev` form and copy the results back.  Both paths run the same kernel
on the same bits, so every comparison here is exact: the host form's float64 arrays and the device outputs widened to float64
are compared through a uint64 view (NaN rows of failed or inactive filters compare as equal bits), integer arrays byte for
byte, covariances through the tests' lower-triangle packing.  No tolerance appears anywhere.

Two engines per run, initialised identically from synth's states (fixed seeds); filter DEAD is left uninitialised, so that a
NaN row and a non-zero status cross the staging path too, every other filter is scored (status 0, asserted).  Capacity 5: one
full group of four filters per wavefront and a partial one; the banks: capacity 6 with 2 hypotheses; windows of 3 steps;
sampled update m = 2; 2 candidates, the association with either point_per_candidate setting; gather / scatter: 3 of 5.

Capacity N_BIG, Pose, either precision: the sensor-frame update with every output and the conditioning (a covariance output)
once more, where the [n][9] arrays (and mean and covariance) are long enough for an fp32 engine to convert them on the device
while the [n][3] and [n] arrays of the same call still convert on the host.

Each form runs twice, for either model and either precision.
  full  every optional input is given per filter and every output is requested, through the Python wrapper.  The optional
        per-filter inputs repeat what the second run's defaults and uniform values say (ids, mount, point, lag, activity,
        latched inputs, the engine's own state), the required ones come from the features' input families
        (sensor_meas_cases / bearing_reference / sampled_reference / predict_sampled_reference / state_meas_reference
        make_inputs, synth's cycle inputs).
  bare  every optional per-filter input and every optional output is NULL (the C function through ctypes, with nulls), the
        device form likewise.  Outputs a form refuses to go without stay (innovation: maha; combine, smooth, forecast: mu;
        sigma points: X).  The call succeeds, the two engines end bit-identical, and -- but for scatter, whose NULL index
        means "item k is filter k" -- in the state the full run left."""
import ctypes as C

import numpy as np
import pytest
import torch

import bearing_reference as br
import predict_sampled_reference as pr
import sampled_reference as sm
import sensor_meas_cases as smc
import sensor_meas_reference as sr
import state_meas_reference as smr
from engine_support import ACC_COV, man_of, new_engine, pack

pytestmark = pytest.mark.gpu

N, DEAD = 5, 2
HYP, N_BANK = 2, 6
STEPS, DT = 3, 0.01
K = 2          # candidates
M = 2          # sampled measurement dimension
# A capacity just past the point where [n][9] arrays hold the 16 384 scalars (ukfb::DEVICE_CONVERT_MIN) from which upload / download
# convert on the device (fp32 engines), while [n][7], [n][3] and [n] stay below: 1 822 * 9 = 16 398, 1 822 * 7 = 12 754.  Not a
# multiple of four: the last wavefront is a partial group.
N_BIG = 1822
ITEMS = np.array([4, DEAD, 0], dtype=np.int32)   # gather / scatter: 3 of 5, the uninitialised filter among them
ST_UNINIT = 1 << 7


# ------------------------------------------------------------------------------------------------------------------ helpers
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(name, host, devt, cov=False):
    """a host-form array against the device buffer: floats through their float64 bits, integers byte for byte"""
    d = devt.detach().cpu().numpy()
    host = np.asarray(host)
    if host.dtype == np.float64:
        if cov:
            assert np.array_equal(bits(host), bits(np.swapaxes(host, -1, -2))), name + ": not symmetric"
            host = pack(host)
        assert np.array_equal(bits(host).reshape(-1), bits(d.astype(np.float64)).reshape(-1)), name
    else:
        if host.dtype == np.bool_:
            host, d = host.astype(np.uint8), (d != 0).astype(np.uint8)
        assert host.dtype.itemsize == d.dtype.itemsize, name
        assert np.array_equal(np.ascontiguousarray(host).view(np.uint8).reshape(-1), np.ascontiguousarray(d).view(np.uint8).reshape(-1)), name


def snap(e):
    mu, cov, init = e.state()
    return mu, cov, init, e.status(), e.last_measurement_time()


def assert_same_engines(name, a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if x.dtype == np.float64:
            assert np.array_equal(bits(x), bits(y)), (name, k)
        else:
            assert np.array_equal(x, y), (name, k)


class Ctx:
    """model, precision, capacity: the states of a fresh engine as downloaded and the shared inputs"""

    def __init__(self, spe, model, prec, n):
        sy = spe.synth
        self.spe, self.model, self.prec, self.n = spe, model, prec, n
        self.man = man_of(model)
        self.S, self.D = (13, 12) if model == "pose" else (14, 13)
        self.PK = self.D * (self.D + 1) // 2
        self.dtype = np.float64 if prec == spe.F64 else np.float32
        self.tdt = torch.float64 if prec == spe.F64 else torch.float32
        self.mu0, self.cov0 = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
        if model == "pose":
            self.acc, self.z, self.Q = sy.pose_cycle_inputs(n, 0, self.mu0[:, :3], random_q=True)
            self.gyro = np.zeros((n, 3))
            self.meas = spe.MEAS_POS3
        else:
            self.gyro, self.acc, self.z, self.Q = sy.orient_cycle_inputs(n, 0, self.mu0[:, :4])
            self.meas = spe.MEAS_ORIENT_BODYVEL3
        e = self.engine()
        self.mu, self.cov, init = e.state()   # as stored; the dead filter's row is whatever the engine holds
        e.close()
        assert list(init) == [i != DEAD for i in range(n)]
        self.mu_f, self.cov_f = self.mu.copy(), self.cov.copy()
        self.mu_f[DEAD], self.cov_f[DEAD] = self.mu[0], self.cov[0]   # (inputs of the dead filter: never used)
        self.alive = np.arange(n) != DEAD

    def engine(self):
        spe, n = self.spe, self.n
        e = new_engine(spe, self.model, n, self.prec, 0)
        for lo, hi in ((0, DEAD), (DEAD + 1, n)):   # every filter but DEAD
            e.initialize(self.mu0[lo:hi], self.cov0[lo:hi], first=lo)
        if self.model == "pose":
            e.set_acceleration(self.acc, ACC_COV)
        else:
            e.set_orient_inputs(self.gyro, self.acc)
        e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
        return e

    # device arrays from the same NumPy inputs, cast to the engine's dtype
    def fl(self, a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(self.dtype))).to("cuda")

    def buf(self, *shape, fill=-7.0):
        return torch.full(shape, fill, dtype=self.tdt, device="cuda")


def it(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")


def ibuf(*shape, dtype=torch.int32):
    return torch.full(shape, 7 if dtype == torch.uint8 else -1, dtype=dtype, device="cuda")


_CTX = {}


def ctx(spe, model, prec, n=N):
    key = (model, prec, n)
    if key not in _CTX:
        _CTX[key] = Ctx(spe, model, prec, n)
    return _CTX[key]


def f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def pd(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def ok(e, rc, what):
    assert rc == 0, (what, rc, e._lib.ukfb_last_error())


def scored(c, status):
    """every initialised filter is scored, the dead one says so"""
    st = np.asarray(status).astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(st, np.where(c.alive, 0, ST_UNINIT)), st


def window(c):
    """a history of STEPS steps recorded from a fresh engine (host arrays as downloaded) and the latched inputs per step"""
    if not hasattr(c, "hist"):
        e = c.engine()
        mus, covs = [], []
        for s in range(STEPS):
            if s:
                e.predict(DT)
            m, cv, _ = e.state()
            mus.append(m); covs.append(cv)
        e.close()
        c.hist = (np.stack(mus), np.stack(covs), np.broadcast_to(c.acc, (STEPS, c.n, 3)).copy(),
                  np.broadcast_to(c.gyro, (STEPS, c.n, 3)).copy())
    return c.hist


def compare(name, host, dev, covs=()):
    for key, t in dev.items():
        if t is not None:
            assert_same(f"{name}/{key}", host[key], t, cov=key in covs)


# ---------------------------------------------------------------------------------------------------------------- the forms
# Each takes (c, eh, ed, full): runs the host-array form on eh and the device form on ed, compares every output.
def form_innovation(c, eh, ed, full):
    n = c.n
    z = np.stack([c.z + 0.01 * k for k in range(K)])
    dev = {"z_pred": c.buf(n, 4), "S": c.buf(n, 9), "innov": c.buf(K, n, 3), "maha": c.buf(K, n), "loglik": c.buf(K, n),
           "best": ibuf(n), "status": ibuf(n)}
    if full:
        host = eh.innovation(c.meas, z, c.Q)
        scored(c, host["status"])
    else:
        dev = {k: (t if k == "maha" else None) for k, t in dev.items()}
        host = {"maha": np.empty((K, n))}
        zz, QQ = f64(z), f64(c.Q)
        ok(eh, eh._lib.ukfb_innovation(eh._h, C.c_int(c.meas), C.c_int(K), pd(zz), pd(QQ), None, None, None, pd(host["maha"]), None,
                                       None, None), "ukfb_innovation")
    ed.innovation_dev(c.meas, K, c.fl(z), c.fl(c.Q.reshape(n, 9)), **dev)
    compare("innovation", host, dev)


def bank_weights(c):
    return np.tile([0.3, 0.7], c.n // HYP)


def form_bank_combine(c, eh, ed, full):
    T, w = c.n // HYP, bank_weights(c)
    dev = {"mu": c.buf(T, c.S), "cov": c.buf(T, c.PK) if full else None, "status": ibuf(T) if full else None}
    if full:
        host = dict(zip(("mu", "cov", "status"), eh.bank_combine(HYP, w)))
        assert list(host["status"] != 0) == [DEAD // HYP == t for t in range(T)]
    else:
        host = {"mu": np.empty((T, c.S))}
        ok(eh, eh._lib.ukfb_bank_combine(eh._h, C.c_int(HYP), pd(f64(w)), pd(host["mu"]), None, None), "ukfb_bank_combine")
    ed.bank_combine_dev(HYP, c.fl(w), dev["mu"], dev["cov"], dev["status"])
    compare("bank_combine", host, dev, covs=("cov",))


def form_bank_mix(c, eh, ed, full):
    T, w = c.n // HYP, bank_weights(c)
    P = f64([[0.9, 0.1], [0.2, 0.8]])
    dev = {"w_pred": c.buf(c.n), "status": ibuf(T) if full else None}
    if full:
        host = dict(zip(("w_pred", "status"), eh.bank_mix(HYP, w, P)))
        assert list(host["status"] != 0) == [DEAD // HYP == t for t in range(T)]
    else:
        host = {"w_pred": np.empty(c.n)}
        ok(eh, eh._lib.ukfb_bank_mix(eh._h, C.c_int(HYP), pd(f64(w)), pd(P), pd(host["w_pred"]), None), "ukfb_bank_mix")
    wt, st = c.fl(w), dev["status"]   # (the wrapper always makes a status buffer: the C function, so that it can go without)
    ok(ed, ed._lib.ukfb_bank_mix_dev(ed._h, C.c_int(HYP), C.c_void_p(wt.data_ptr()), pd(P), C.c_void_p(dev["w_pred"].data_ptr()),
                                     None if st is None else C.cast(st.data_ptr(), C.POINTER(C.c_uint32))), "ukfb_bank_mix_dev")
    compare("bank_mix", host, dev)


def form_smooth(c, eh, ed, full):
    mu_h, cov_h, a, b = window(c)
    dt = np.full(STEPS - 1, DT)
    mu_t, cov_t, st = c.fl(mu_h), c.fl(pack(cov_h)), (ibuf(c.n) if full else None)
    if full:
        host = dict(zip(("mu", "cov", "status"), eh.smooth(dt, mu_h, cov_h, a, b)))
        scored_window(c, host["status"])
    else:
        host = {"mu": mu_h.copy(), "cov": cov_h.copy()}
        ok(eh, eh._lib.ukfb_smooth(eh._h, C.c_int(STEPS), pd(dt), pd(host["mu"]), pd(host["cov"]), None, None, None), "ukfb_smooth")
    ed.smooth_dev(dt, STEPS, 0, mu_t, cov_t, status=st, in_a_dev=c.fl(a) if full else None, in_b_dev=c.fl(b) if full else None)
    compare("smooth", host, {"mu": mu_t, "cov": cov_t, "status": st}, covs=("cov",))


def scored_window(c, status):
    """the window features take the dead filter's record as it lies in the history: only the live filters are held to 0"""
    st = np.asarray(status).astype(np.int64) & 0xFFFFFFFF
    assert (st[c.alive] == 0).all(), st


def form_forecast(c, eh, ed, full):
    n = c.n
    _, _, a, b = window(c)
    dt = np.full(STEPS, DT)
    dev = {"mu": c.buf(STEPS, n, c.S, fill=0.0), "cov": c.buf(STEPS, n, c.PK, fill=0.0) if full else None,
           "status": ibuf(n) if full else None}
    if full:
        host = dict(zip(("mu", "cov", "status"), eh.forecast(dt=dt, start_mu=c.mu, start_cov=c.cov, in_a=a, in_b=b)))
        scored(c, host["status"])
    else:
        host = {"mu": np.zeros((STEPS, n, c.S))}
        ok(eh, eh._lib.ukfb_forecast(eh._h, C.c_int(STEPS), pd(dt), None, None, None, None, None, pd(host["mu"]), None, None), "ukfb_forecast")
    ed.forecast_dev(STEPS, 0, dev["mu"], dev["cov"], dev["status"], dt=dt, start_mu=c.fl(c.mu) if full else None,
                    start_cov=c.fl(pack(c.cov)) if full else None, in_a_dev=c.fl(a) if full else None, in_b_dev=c.fl(b) if full else None)
    compare("forecast", host, dev, covs=("cov",))


def form_gather(c, eh, ed, full):
    m = len(ITEMS)
    if full:
        host = dict(zip(("mu", "cov", "last_ts_us", "initialised"), eh.gather_filters(ITEMS)))
        assert list(host["initialised"]) == [i != DEAD for i in ITEMS]
        dev = {"mu": c.buf(m, c.S), "cov": c.buf(m, c.PK), "last_ts_us": ibuf(m, dtype=torch.int64), "initialised": ibuf(m, dtype=torch.uint8)}
        ed.gather_filters_dev(it(ITEMS, np.int32), mu=dev["mu"], cov_packed=dev["cov"], last_ts_us=dev["last_ts_us"], initialised=dev["initialised"])
        compare("gather", host, dev, covs=("cov",))
    else:
        ok(eh, eh._lib.ukfb_gather_filters(eh._h, C.c_int64(c.n), None, None, None, None, None), "ukfb_gather_filters")
        ed.gather_filters_dev(None)


def form_scatter(c, eh, ed, full):
    m = len(ITEMS) if full else c.n
    mu, cov = c.mu_f[::-1][:m].copy(), (1.5 * c.cov_f[::-1][:m]).copy()
    if full:
        ts, init = np.array([11, 22, 33], dtype=np.int64), np.array([1, 1, 0], dtype=np.uint8)
        host = {"status": eh.scatter_filters(ITEMS, mu, cov, last_ts_us=ts, initialised=init)}
        assert (host["status"] == 0).all()
        dev = {"status": ibuf(m)}
        ed.scatter_filters_dev(it(ITEMS, np.int32), c.fl(mu), c.fl(pack(cov)), last_ts_us=it(ts, np.int64), initialised=it(init, np.uint8),
                               status=dev["status"])
        compare("scatter", host, dev)
    else:
        ok(eh, eh._lib.ukfb_scatter_filters(eh._h, C.c_int64(m), None, pd(mu), pd(cov), None, None, None), "ukfb_scatter_filters")
        ed.scatter_filters_dev(None, c.fl(mu), c.fl(pack(cov)))


def form_compact(c, eh, ed, full):
    if full:
        new, old, live = eh.compact(1)
        assert live == c.n - 1
        host = {"new_index": new, "old_index": old, "live": np.array([live], dtype=np.int64)}
        dev = {"new_index": ibuf(c.n), "old_index": ibuf(c.n), "live": ibuf(1, dtype=torch.int64)}
        ed.compact_dev(1, dev["new_index"], dev["old_index"], dev["live"])
        compare("compact", host, dev)
    else:
        ok(eh, eh._lib.ukfb_compact(eh._h, C.c_int(1), None, None, None), "ukfb_compact")
        ed.compact_dev(1)


def form_update_state(c, eh, ed, full):
    n = c.n
    if not hasattr(c, "state_meas"):
        c.state_meas = smr.make_inputs(c.man, c.mu_f, c.cov_f, c.dtype)
    z, Qz = c.state_meas
    mask = c.spe.BLOCK_POSE_ALL if c.model == "pose" else c.spe.BLOCK_ORIENT_ALL
    if full:
        host = dict(zip(("maha", "loglik", "status"), eh.update_state(np.full(n, mask, dtype=np.int32), z, Qz)))
        scored(c, host["status"])
        dev = {"maha": c.buf(n), "loglik": c.buf(n), "status": ibuf(n)}
        ed.update_state_dev(0, c.fl(z), c.fl(pack(Qz)), block_mask_dev=it(np.full(n, mask), np.int32), **dev)
        compare("update_state", host, dev)
    else:
        zz, QQ = f64(z), f64(Qz)
        ok(eh, eh._lib.ukfb_update_state(eh._h, C.c_uint32(mask), None, pd(zz), pd(QQ), C.c_double(1.0), C.c_double(1.0), C.c_int(1), None,
                                         None, None), "ukfb_update_state")
        ed.update_state_dev(mask, c.fl(z), c.fl(pack(Qz)))


def sensor_inputs(c, bearing):
    """(model id, z [n, 3], Q, mount [7], point [3]): the family's z and Q per filter, the first filter's mount and point for all"""
    key = "bearing_in" if bearing else "sensor_in"
    if not hasattr(c, key):
        if bearing:
            mid = br.POSE_POINT if c.model == "pose" else br.ORIENT_NAV_DIRECTION
            mount, point, z, Q = br.make_inputs(c.man, c.mu_f, 15.0, 80.0, c.dtype)
        else:
            mid = sr.POSE_POINT if c.model == "pose" else sr.ORIENT_NAV_VECTOR
            mount, point, _, z, Q = smc.make_inputs(c.model, c.mu_f, c.dtype)
        setattr(c, key, (mid, z[mid], Q, mount[0].copy(), point[0].copy()))
    return getattr(c, key)


def form_sensor_frame(c, eh, ed, full, bearing):
    n = c.n
    mid, z, Q, mount, point = sensor_inputs(c, bearing)
    fn = "ukfb_update_bearing" if bearing else "ukfb_update_sensor"
    if full:
        ids, mounts, points = np.full(n, mid, dtype=np.int32), np.tile(mount, (n, 1)), np.tile(point, (n, 1))
        host = (eh.update_bearing if bearing else eh.update_sensor)(ids, z, Q, mounts, points)
        scored(c, host["status"])
        dev = {"z_pred": c.buf(n, 3), "S": c.buf(n, 9), "innov": c.buf(n, 3), "maha": c.buf(n), "loglik": c.buf(n), "status": ibuf(n)}
        (ed.update_bearing_dev if bearing else ed.update_sensor_dev)(0, c.fl(z), c.fl(Q.reshape(n, 9)), model_dev=it(ids, np.int32),
                                                                      mount_dev=c.fl(mounts), point_dev=c.fl(points), **dev)
        compare(fn, host, dev)
    else:
        zz, QQ, mm, pp = f64(z), f64(Q), f64(mount), f64(point)
        ok(eh, getattr(eh._lib, fn)(eh._h, C.c_int(mid), None, pd(zz), pd(QQ), None, pd(mm), None, pd(pp), C.c_int(1), None, None, None,
                                    None, None, None), fn)
        (ed.update_bearing_dev if bearing else ed.update_sensor_dev)(mid, c.fl(z), c.fl(Q.reshape(n, 9)), mount=mount, point=point)


def form_update_sensor(c, eh, ed, full):
    form_sensor_frame(c, eh, ed, full, False)


def form_update_bearing(c, eh, ed, full):
    form_sensor_frame(c, eh, ed, full, True)


def form_associate(c, eh, ed, full, per_candidate):
    n = c.n
    mid, z1, Q, mount, point = sensor_inputs(c, False)
    z = np.stack([z1 + 0.01 * k for k in range(K)])
    H = K if per_candidate else 1
    points = np.stack([np.tile(point, (n, 1)) + 0.1 * k for k in range(K)]) if per_candidate else np.tile(point, (n, 1))
    if full:
        ids, mounts = np.full(n, mid, dtype=np.int32), np.tile(mount, (n, 1))
        host = eh.associate_sensor(ids, z, Q, mounts, points, point_per_candidate=per_candidate)
        scored(c, host["status"])
        dev = {"z_pred": c.buf(H, n, 3), "S": c.buf(H, n, 9), "innov": c.buf(K, n, 3), "maha": c.buf(K, n), "loglik": c.buf(K, n),
               "best": ibuf(n), "n_gated": ibuf(n), "status": ibuf(n)}
        ed.associate_sensor_dev(0, K, c.fl(z), c.fl(Q.reshape(n, 9)), model_dev=it(ids, np.int32), mount_dev=c.fl(mounts),
                                point_dev=c.fl(points), point_per_candidate=per_candidate, **dev)
        compare("associate", host, dev)
    else:   # (per candidate the point array is required; shared, the point is the uniform value)
        zz, QQ, mm, pp = f64(z), f64(Q), f64(mount), f64(points if per_candidate else point)
        ok(eh, eh._lib.ukfb_associate_sensor(eh._h, C.c_int(mid), None, C.c_int(K), pd(zz), pd(QQ), None, pd(mm),
                                             pd(pp) if per_candidate else None, None if per_candidate else pd(pp),
                                             C.c_int(1 if per_candidate else 0), C.c_int(1), None, None, None, None, None, None, None, None),
           "ukfb_associate_sensor")
        if per_candidate:
            ed.associate_sensor_dev(mid, K, c.fl(z), c.fl(Q.reshape(n, 9)), mount=mount, point_dev=c.fl(points), point_per_candidate=True)
        else:
            ed.associate_sensor_dev(mid, K, c.fl(z), c.fl(Q.reshape(n, 9)), mount=mount, point=point)


def form_associate_shared(c, eh, ed, full):
    form_associate(c, eh, ed, full, False)


def form_associate_per_candidate(c, eh, ed, full):
    form_associate(c, eh, ed, full, True)


def exported_points(c):
    """X [n, 2 D + 1, S] of a fresh engine, as the host form downloads it (the dead filter's rows are NaN)"""
    if not hasattr(c, "X"):
        e = c.engine()
        c.X, _, st = e.sigma_points()
        e.close()
        scored(c, st)
    return c.X


def form_sigma_points(c, eh, ed, full):
    n, pts = c.n, 2 * c.D + 1
    dev = {"X": c.buf(n, pts, c.S), "delta": c.buf(n, pts, c.D) if full else None, "status": ibuf(n) if full else None}
    if full:
        host = dict(zip(("X", "delta", "status"), eh.sigma_points()))
        scored(c, host["status"])
        assert np.isnan(host["X"][DEAD]).all()
    else:
        host = {"X": np.empty((n, pts, c.S))}
        ok(eh, eh._lib.ukfb_sigma_points(eh._h, pd(host["X"]), None, None), "ukfb_sigma_points")
    ed.sigma_points_dev(dev["X"], dev["delta"], dev["status"])
    compare("sigma_points", host, dev)


def form_update_sampled(c, eh, ed, full):
    n = c.n
    if not hasattr(c, "sampled_in"):
        b, r, noise, Q = sm.make_inputs(c.model, c.mu_f, c.dtype)
        Z = sm.user_h(c.model, M, exported_points(c), b[:, None, :], r[:, None, :])
        c.sampled_in = (Z, sm.user_h(c.model, M, c.mu_f, b, r) + noise[M], Q[M])
    Z, z, Q = c.sampled_in
    if full:
        active = np.ones(n, dtype=np.uint8)
        host = eh.update_sampled(Z, z, Q, active=active)
        scored(c, host["status"])
        dev = {"z_pred": c.buf(n, M), "S": c.buf(n, M, M), "innov": c.buf(n, M), "maha": c.buf(n), "loglik": c.buf(n), "status": ibuf(n)}
        ed.update_sampled_dev(M, c.fl(Z), c.fl(z), c.fl(Q), active_dev=it(active, np.uint8), **dev)
        compare("update_sampled", host, dev)
    else:
        ZZ, zz, QQ = f64(Z), f64(z), f64(Q)
        ok(eh, eh._lib.ukfb_update_sampled(eh._h, C.c_int(M), pd(ZZ), pd(zz), pd(QQ), C.c_int(0), None, C.c_int(1), None, None, None, None,
                                           None, None), "ukfb_update_sampled")
        ed.update_sampled_dev(M, c.fl(Z), c.fl(z), c.fl(Q))


def form_predict_sampled(c, eh, ed, full):
    n = c.n
    if not hasattr(c, "predict_in"):
        par, R = pr.make_inputs(c.model, c.mu_f, c.dtype)
        name = "drag" if c.model == "pose" else "markov"
        c.predict_in = (pr.user_f(c.model, name, exported_points(c), pr.expand(par[name])), R)
    XX, R = c.predict_in
    if full:
        active = np.ones(n, dtype=np.uint8)
        host = eh.predict_sampled(XX, R, active=active)
        scored(c, host["status"])
        dev = {"mu": c.buf(n, c.S), "cov": c.buf(n, c.PK), "status": ibuf(n)}
        ed.predict_sampled_dev(c.fl(XX), c.fl(R), active_dev=it(active, np.uint8), mu=dev["mu"], cov_packed=dev["cov"], status=dev["status"])
        compare("predict_sampled", host, dev, covs=("cov",))
    else:
        XXc, RR = f64(XX), f64(R)
        ok(eh, eh._lib.ukfb_predict_sampled(eh._h, pd(XXc), pd(RR), C.c_int(0), None, C.c_int(1), None, None, None), "ukfb_predict_sampled")
        ed.predict_sampled_dev(c.fl(XX), c.fl(R))


def form_condition(c, eh, ed, full):
    n = c.n
    floor = np.linspace(1e-7, 2e-7, c.D)
    floor[0] = 1.0   # above every filter's first variance: each one is repaired, so the call commits something
    eps = 1e-10 if c.prec == c.spe.F64 else 1e-4
    if full:
        select = np.ones(n, dtype=np.uint8)
        host = eh.condition(floor, eps, select=select, renormalize_quaternion=True)
        st = host["status"].astype(np.int64)
        assert ((st[c.alive] & ~c.spe.ST_REPAIRED) == 0).all() and st[DEAD] == ST_UNINIT, st
        dev = {"eig_min": c.buf(n), "eig_max": c.buf(n), "mu": c.buf(n, c.S), "cov": c.buf(n, c.PK), "status": ibuf(n)}
        ed.condition_dev(c.fl(floor), eps, select_dev=it(select, np.uint8), renormalize_quaternion=True, eig_min=dev["eig_min"],
                         eig_max=dev["eig_max"], mu=dev["mu"], cov_packed=dev["cov"], status=dev["status"])
        compare("condition", host, dev, covs=("cov",))
    else:
        ff = f64(floor)
        ok(eh, eh._lib.ukfb_condition(eh._h, pd(ff), C.c_double(eps), None, C.c_int(1), C.c_int(1), None, None, None, None, None),
           "ukfb_condition")
        ed.condition_dev(c.fl(floor), eps, renormalize_quaternion=True)


def form_update_delayed(c, eh, ed, full):
    n, lag = c.n, 1
    mu_h, cov_h, a, b = window(c)
    dt = np.full(STEPS - 1, DT)
    for e in (eh, ed):   # the window's last step is the engine's own state
        for _ in range(STEPS - 1):
            e.predict(DT)
    if full:
        lags, ids = np.full(n, lag, dtype=np.int32), np.full(n, c.meas, dtype=np.int32)
        host = eh.update_delayed(dt, mu_h, cov_h, lags, ids, c.z, c.Q, in_a=a, in_b=b)
        scored_window(c, host["status"])
        dev = {"z_pred": c.buf(n, 4), "S": c.buf(n, 9), "innov": c.buf(n, 3), "maha": c.buf(n), "loglik": c.buf(n), "status": ibuf(n),
               "mu_out": c.buf(n, c.S), "cov_out": c.buf(n, c.PK)}
        ed.update_delayed_dev(dt, STEPS, 0, c.fl(mu_h), c.fl(pack(cov_h)), it(lags, np.int32), it(ids, np.int32), c.fl(c.z),
                              c.fl(c.Q.reshape(n, 9)), in_a_dev=c.fl(a), in_b_dev=c.fl(b), **dev)
        compare("update_delayed", host, dev, covs=("cov_out",))
    else:
        mm, cc, zz, QQ = f64(mu_h), f64(cov_h), f64(c.z), f64(c.Q)
        ok(eh, eh._lib.ukfb_update_delayed(eh._h, C.c_int(STEPS), pd(dt), pd(mm), pd(cc), None, None, C.c_int(lag), None, C.c_int(c.meas),
                                           None, pd(zz), pd(QQ), C.c_int(1), None, None, None, None, None, None, None, None),
           "ukfb_update_delayed")
        ed.update_delayed_dev(dt, STEPS, 0, c.fl(mu_h), c.fl(pack(cov_h)), lag, c.meas, c.fl(c.z), c.fl(c.Q.reshape(n, 9)))


# name -> (function, capacity, commits, the bare run ends where the full run ends)
FORMS = {
    "innovation": (form_innovation, N, False, True),
    "bank_combine": (form_bank_combine, N_BANK, False, True),
    "bank_mix": (form_bank_mix, N_BANK, True, True),
    "smooth": (form_smooth, N, False, True),
    "forecast": (form_forecast, N, False, True),
    "gather_filters": (form_gather, N, False, True),
    "scatter_filters": (form_scatter, N, True, False),
    "compact": (form_compact, N, True, True),
    "update_state": (form_update_state, N, True, True),
    "update_sensor": (form_update_sensor, N, True, True),
    "update_bearing": (form_update_bearing, N, True, True),
    "associate_sensor-shared": (form_associate_shared, N, True, True),
    "associate_sensor-per-candidate": (form_associate_per_candidate, N, True, True),
    "sigma_points": (form_sigma_points, N, False, True),
    "update_sampled": (form_update_sampled, N, True, True),
    "predict_sampled": (form_predict_sampled, N, True, True),
    "condition": (form_condition, N, True, True),
    "update_delayed": (form_update_delayed, N, True, True),
}


@pytest.mark.parametrize("prec", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("form", list(FORMS))
def test_host_form_is_device_form(spe, form, model, prec):
    fn, n, commits, same_end = FORMS[form]
    c = ctx(spe, model, prec, n)
    ends = {}
    for full in (True, False):
        eh, ed = c.engine(), c.engine()
        before = snap(eh)
        assert_same_engines(f"{form}: twins", before, snap(ed))
        fn(c, eh, ed, full)
        ed.sync()
        torch.cuda.synchronize()
        ends[full] = snap(eh)
        assert_same_engines(f"{form}: host against device engine, full={full}", ends[full], snap(ed))
        if commits and form != "update_delayed":   # (the delayed update's engines have also predicted)
            assert not all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, ends[full])), f"{form} committed nothing"
        eh.close(); ed.close()
    if same_end:
        assert_same_engines(f"{form}: bare run against full run", ends[True], ends[False])


@pytest.mark.parametrize("prec", [0, 1], ids=["f64", "f32"])
def test_host_form_is_device_form_across_the_conversion_threshold(spe, prec):
    """update_sensor with every output (z, mount, point, innov, maha, loglik below the threshold; Q, S above it) and condition (its
    covariance output staged through cov_out, above it) at capacity N_BIG: bit for bit the device form"""
    assert N_BIG * 7 < 16384 <= N_BIG * 9 < 16384 + 2 * 9 and N_BIG % 4 != 0
    c = ctx(spe, "pose", prec, N_BIG)
    for name, fn in (("update_sensor", form_update_sensor), ("condition", form_condition)):
        eh, ed = c.engine(), c.engine()
        before = snap(eh)
        assert_same_engines(f"{name}: twins", before, snap(ed))
        fn(c, eh, ed, True)
        ed.sync()
        torch.cuda.synchronize()
        end = snap(eh)
        assert_same_engines(f"{name}: host against device engine", end, snap(ed))
        assert not all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, end)), f"{name} committed nothing"
        eh.close(); ed.close()
