"""40-digit references, deterministic case tables and error units for the measurement-side device primitives of the sensor-frame,
bearing, association and sampled kernels: s2_log, s2_exp, bearing_h (ukf_bearing.hpp), cos_sinc_sqrt (ukf_device.hpp), sensor_h,
sensor_solve3 (ukf_sensor_meas.hpp) and sampled_solve6 (ukf_sampled.hpp).  A helper with no GPU dependency and no tests:
tests/test_meas_primitives_reference.py holds the NumPy statements the parity tests rely on to these references, and
tests/test_gpu_meas_primitives.py the device (tests/cpp/meas_probe.hip).

References (mpmath, 40 digits, from the exact binary inputs; definitions of include/ukf_batch.h):
  s2_log    theta = atan2(|u x v|, u.v), direction of v - (u.v) u; zeros where that vector is zero
  s2_exp    cos|w| u + sinc|w| w, normalised
  cos_sinc  cos sqrt x2, sin sqrt x2 / sqrt x2
  models    true rotations, R(q) of the normalised quaternion; the inverses the device takes as inputs (qsi = conj(qs) / |qs|^2,
            rnq = 1 / |q|^2) are formed here on the host in float64 and belong to the record
  solves    forward substitution with Ls[r][k] = lf[r (r + 1) / 2 + k] rs[k] (k < r), Ls[k][k] = 1 / rs[k], built from the rounded
            lf and rs (sensor_solve3: Ls[r][k] = l_rk as passed)

Error units, eps = eps(T); `unit` is what multiplies eps, `recip` the size of the result that a hardware-seeded reciprocal of the
device code scales (the second term of the bound, tests/test_gpu_meas_primitives.py):
  s2_log    max(1, theta_ref / |t_ref|), absolute;  recip |w_ref|
  s2_exp    1, absolute;                            recip 1
  cos_sinc  1, absolute
  bearing_h (|b - p| + |r|) / |d_ref|;              recip 1
  sensor_h  the sum of the norms of the operands the model adds
  solves    (|Ls^-1| |Ls| |y|)_k, componentwise

A table is a Table: X the device records [n, IN], reg the regime of every record (index into names), cls the classes between
which the neighbour-independence test mixes records (regimes or model ids), raw the inputs as the NumPy statements take them."""
import functools
import os
from types import SimpleNamespace

import numpy as np

from probe_support import DT, EPS, F32, F64, _axes, _m, _ulps

IN, OUT = 33, 6                       # doubles per record (tests/cpp/meas_probe.hip MEASP_IN / MEASP_OUT)
MR_ID, MR_R, MR_QSI, MR_B, MR_GY, MR_RNQ = 14, 15, 18, 22, 25, 28
PRIM = dict(s2_log=0, s2_exp=1, cos_sinc_sqrt=2, bearing_pose=3, bearing_orient=4, sensor_pose=5, sensor_orient=6, solve3=7, solve6=8)
NOUT = dict(s2_log=3, s2_exp=3, cos_sinc_sqrt=2, bearing_pose=3, bearing_orient=3, sensor_pose=3, sensor_orient=3, solve3=3, solve6=6)
IN_T = ("cos_sinc_sqrt", "solve3", "solve6")          # run in T = double and float; the rest are fp64 in every mode
TAYLOR = {F64: 0.0001220703125, F32: float(np.float32(0.018581361))}    # Num<T>::taylor_n_bound (ukf_device.hpp)
RECIP = {F64: 24.0, F32: 2.0}         # fast_rsqrt / fast_rcp, relative, in eps(T): the bounds of tests/test_gpu_so3_primitives.py
SENTINEL = 12345.5                    # c[k] beyond m holds SENTINEL + k (exact in float)
RANGES = (1e-3, 1.0, 50.0, 1e4, 1e7)
SENSOR_NAMES = ("POSE_POSITION", "POSE_RANGE", "POSE_POINT", "POSE_VELOCITY", "POSE_NAV_VELOCITY", "ORIENT_VELOCITY", "ORIENT_NAV_VECTOR",
                "ORIENT_SPECIFIC_FORCE")
READS_LEVER, READS_ROTATION, READS_POINT = (0, 1, 2, 3, 5), (2, 3, 5, 6), (1, 2, 6)    # tests/sensor_meas_reference.py


def mp():
    import mpmath
    return mpmath


def Table(X, reg, names, cls=None, **raw):
    reg = np.asarray(reg, dtype=np.int64)
    return SimpleNamespace(X=np.ascontiguousarray(X, dtype=np.float64), reg=reg, names=tuple(names),
                           cls=reg if cls is None else np.asarray(cls, dtype=np.int64), raw=SimpleNamespace(**raw))


# ------------------------------------------------------------------------------------------------ small mpmath vector algebra
def _v(x):
    return [_m(a) for a in x]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(a):
    return mp().sqrt(_dot(a, a))


def _rot(q, x):
    """R(q) x for the normalised quaternion (x, y, z, w)"""
    n = _norm(q)
    u, w = [a / n for a in q[:3]], q[3] / n
    a = _cross(u, x)
    b = _cross(u, a)
    return [x[i] + 2 * (w * a[i] + b[i]) for i in range(3)]


def _rot_t(q, x):
    return _rot([-q[0], -q[1], -q[2], q[3]], x)


def _pairs(vals, n):
    """(hi, lo) [n, OUT] of a list of rows of mp values"""
    hi, lo = np.zeros((n, OUT)), np.zeros((n, OUT))
    for i, row in enumerate(vals):
        for k, v in enumerate(row):
            h = float(v)
            hi[i, k] = h
            lo[i, k] = float(v - h) if np.isfinite(h) else 0.0
    return hi, lo


# ------------------------------------------------------------------------------------------------ the sphere maps
LOG_REGIMES = ("same", "small", "mid", "near_pi", "antipode", "offunit", "nan")
LOG_SMALL = (1e-12, 1e-9, 1e-6, 1e-3)
LOG_MID = (0.1, 1.0, 0.5 * np.pi, 2.0, 3.0)
EXP_REGIMES = ("tiny", "edge", "mid", "wide")


def _unit_mp(u):
    """the unit vector along u, rounded to double once"""
    with mp().workdps(60):
        x = _v(u)
        n = _norm(x)
        return np.array([float(a / n) for a in x])


def _tangent(rng, u):
    a = rng.normal(size=3)
    a -= np.dot(a, u) * u / np.dot(u, u)
    return a / np.linalg.norm(a)


def _at_angle(u, a, th):
    """cos(th) u + sin(th) a' for th given as an mp expression, a' the unit tangent at u along a (made orthogonal to u at full
    precision, so that the point is a unit vector to its rounding), rounded to double once"""
    uu, aa = _v(u), _v(a)
    k = _dot(aa, uu) / _dot(uu, uu)
    aa = [aa[i] - k * uu[i] for i in range(3)]
    n = _norm(aa)
    return np.array([float(mp().cos(th) * uu[i] + mp().sin(th) * aa[i] / n) for i in range(3)])


def _sphere_points(seed):
    """the base points u: random, +-e_i, (0.6, 0.8, 0), |u0| at 0.6 +- 3 ulp (the axis switch of the antipode branch)"""
    rng = np.random.default_rng(seed)
    us = [_unit_mp(a) for a in rng.normal(size=(4, 3))]
    for i in range(3):
        for s in (1.0, -1.0):
            e = np.zeros(3)
            e[i] = s
            us.append(e)
    us.append(np.array([0.6, 0.8, 0.0]))
    generic = len(us)
    for k, u0 in enumerate(_ulps(0.6, 3, np.float64)):
        rest = np.sqrt(1.0 - float(u0) ** 2)
        us.append(np.array([float(u0) if k % 2 == 0 else -float(u0), rest * 0.6, rest * 0.8]))
    return us, generic, rng


@functools.lru_cache(maxsize=None)
def log_table(seed=2026):
    us, _, rng = _sphere_points(seed)
    rows, reg = [], []

    def add(u, v, name):
        r = np.zeros(IN)
        r[0:3], r[3:6] = u, v
        rows.append(r)
        reg.append(LOG_REGIMES.index(name))

    with mp().workdps(60):
        for u in us:
            a = _tangent(rng, u)
            add(u, u, "same")
            for th in LOG_SMALL:
                add(u, _at_angle(u, a, _m(th)), "small")
            for th in LOG_MID:
                add(u, _at_angle(u, a, _m(th)), "mid")
            for k in range(1, 9):
                add(u, _at_angle(u, a, mp().pi - mp().mpf(10) ** -k), "near_pi")
            add(u, -u, "antipode")
        add(np.array([1.0, 0.0, 0.0]), np.array([1.0, 1e-170, 0.0]), "small")           # t2 underflows
        for u in us[:4]:
            a = _tangent(rng, u)
            for th in (1e-3, 1.0, 3.0):
                v = _at_angle(u, a, _m(th))
                for ku, kv in ((4, 0), (-4, 0), (0, 4), (0, -4), (4, -4)):
                    add(u * (1.0 + ku * 2.0 ** -53), v * (1.0 + kv * 2.0 ** -53), "offunit")
        for u in us[:3]:
            v = _at_angle(u, _tangent(rng, u), _m(1.0))
            for i in range(3):
                un, vn = u.copy(), v.copy()
                un[i] = np.nan
                vn[i] = np.nan
                add(un, v, "nan")
                add(u, vn, "nan")
    return Table(np.array(rows), reg, LOG_REGIMES)


def log_reference(tb):
    """(hi, lo, unit [n, 1], recip [n], theta [n]); the NaN records: NaN"""
    vals, unit, theta = [], [], []
    nan = mp().mpf("nan")
    with mp().workdps(150):   # t loses up to 12 digits to cancellation, (1, 1e-170, 0) none: the exponent range is unbounded
        for r in tb.X:
            if not np.isfinite(r[:6]).all():
                vals.append([nan] * 3)
                unit.append(1.0)
                theta.append(np.nan)
                continue
            u, v = _v(r[0:3]), _v(r[3:6])
            c = _dot(u, v)
            if np.array_equal(r[3:6], -r[0:3]):   # the exact antipode: the direction is unspecified, the length is pi
                vals.append([nan] * 3)
                unit.append(1.0)
                theta.append(float(mp().atan2(0, c)))
                continue
            t = [v[i] - c * u[i] for i in range(3)]
            th = mp().atan2(_norm(_cross(u, v)), c)
            nt = _norm(t)
            vals.append([th * a / nt for a in t] if nt != 0 else [mp().mpf(0)] * 3)
            unit.append(max(1.0, float(th / nt)) if nt != 0 else 1.0)
            theta.append(float(th))
    hi, lo = _pairs(vals, len(tb.X))
    theta = np.array(theta)
    return hi, lo, np.array(unit)[:, None], theta, theta


def _w_lengths(prec=F64):
    """(|w|, regime) of the exponential's table"""
    out = [(0.0, 0), (1e-160, 0), (1e-12, 0), (1e-8, 0), (1e-4, 0)]
    out += [(float(x), 1) for x in _ulps(np.sqrt(TAYLOR[prec]), 4, np.float64)]
    out += [(x, 2) for x in (0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0)]
    out += [(x, 3) for x in (np.pi - 1e-3, np.pi + 1e-3, 4.0, 6.0, 2.0 * np.pi, 10.0)]
    return out


@functools.lru_cache(maxsize=None)
def exp_table(seed=2027):
    us, generic, rng = _sphere_points(seed)
    rows, reg = [], []
    for u in us[:generic]:
        for n, g in _w_lengths():
            r = np.zeros(IN)
            r[0:3], r[3:6] = u, n * _tangent(rng, u)
            rows.append(r)
            reg.append(g)
    for n, g in _w_lengths():   # along an axis: x2 is the rounded square, on both sides of the Taylor switch
        r = np.zeros(IN)
        r[0:3], r[3:6] = [0.0, 0.0, 1.0], [n, 0.0, 0.0]
        rows.append(r)
        reg.append(g)
    return Table(np.array(rows), reg, EXP_REGIMES)


def _cos_sinc_mp(x2):
    if x2 == 0:
        return mp().mpf(1), mp().mpf(1)
    x = mp().sqrt(x2)
    return mp().cos(x), mp().sin(x) / x


def exp_reference(tb):
    vals = []
    with mp().workdps(60):
        for r in tb.X:
            u, w = _v(r[0:3]), _v(r[3:6])
            c, s = _cos_sinc_mp(_dot(w, w))
            e = [c * u[i] + s * w[i] for i in range(3)]
            n = _norm(e)
            vals.append([a / n for a in e])
    hi, lo = _pairs(vals, len(tb.X))
    n = len(tb.X)
    return hi, lo, np.ones((n, 1)), np.ones(n)


CS_REGIMES = ("taylor", "closed", "wide")


@functools.lru_cache(maxsize=None)
def cos_sinc_table(prec):
    T = DT[prec]
    xs = [0.0, float(np.finfo(T).tiny), 1e-160 ** 2, 1e-12 ** 2, 1e-8 ** 2, 1e-4 ** 2]
    xs += [float(x) for x in _ulps(TAYLOR[prec], 3, T)]
    xs += [x * x for x in (0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, np.pi - 1e-3, np.pi + 1e-3, 4.0, 6.0, 2.0 * np.pi, 10.0)]
    x2 = np.unique(np.asarray(xs, dtype=T).astype(np.float64))
    X = np.zeros((len(x2), IN))
    X[:, 0] = x2
    reg = np.where(x2 < TAYLOR[prec], 0, np.where(x2 <= 9.5, 1, 2))
    return Table(X, reg, CS_REGIMES)


def cos_sinc_reference(tb):
    with mp().workdps(60):
        vals = [list(_cos_sinc_mp(_m(r[0]))) for r in tb.X]
    hi, lo = _pairs(vals, len(tb.X))
    return hi, lo, np.ones((len(tb.X), 1)), np.zeros(len(tb.X))


def np_cos_sinc_sqrt(x2, T):
    """MTK's cos_sinc_sqrt in T: three Taylor pairs below eps^(1/4), cos and sin / x above"""
    x2 = np.asarray(x2, dtype=T)
    term = T(-0.5) * x2
    cosi = T(1) + term
    term = term * T(1 / 3.)
    sinc = T(1) + term
    term = term * (T(-1 / 4.) * x2)
    cosi = cosi + term
    term = term * T(1 / 5.)
    sinc = sinc + term
    term = term * (T(-1 / 6.) * x2)
    cosi = cosi + term
    term = term * T(1 / 7.)
    sinc = sinc + term
    x = np.sqrt(x2)
    big = x2 >= T(TAYLOR[F64 if T is np.float64 else F32])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(big, np.cos(x), cosi).astype(T), np.where(big, np.sin(x) / x, sinc).astype(T)


# ------------------------------------------------------------------------------------------------ the models
BEARING_REGIMES = tuple(f"{r:g}" for r in RANGES) + ("cancel", "flag")


def _quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _mounts(rng):
    """(lever arm, qs): identity, random and 180-degree mounts, lever arms of 0 and 0.5 m"""
    a = _axes(rng, 1)[0]
    qss = [np.array([0.0, 0.0, 0.0, 1.0]), _quat(rng), np.array([1.0, 0.0, 0.0, 0.0]), np.array([a[0], a[1], a[2], 0.0])]
    out = []
    for k, qs in enumerate(qss):
        for lever in (0.0, 0.5):
            out.append((lever * _axes(rng, 1)[0], qs))
    return out


def _qsi(qs):
    return qs * np.array([-1.0, -1.0, -1.0, 1.0]) / np.dot(qs, qs)


def _record(x, q, idv, r, qs, b, gy=(0.0, 0.0, 0.0)):
    rec = np.zeros(IN)
    rec[:len(x)] = x
    rec[MR_ID] = idv
    rec[MR_R:MR_R + 3], rec[MR_QSI:MR_QSI + 4], rec[MR_B:MR_B + 3], rec[MR_GY:MR_GY + 3] = r, _qsi(qs), b, gy
    rec[MR_RNQ] = 1.0 / np.dot(q, q)
    return rec


def _pose_state(rng, rate):
    """positions of order 100 m, velocities and rates of order `rate`"""
    return np.concatenate([100.0 * rng.normal(size=3), _quat(rng), rate * rng.normal(size=3), rate * rng.normal(size=3)])


def _orient_state(rng, rate):
    return np.concatenate([_quat(rng), rate * rng.normal(size=3), 0.01 * rate * rng.normal(size=3), 0.1 * rng.normal(size=3),
                           [9.81 + 0.01 * rng.normal()]])


def _cancel_point(x, r, rel):
    """b with R(q)^T (b - p) = r + delta, |delta| = rel (|b - p| + |r|): the lever arm cancels all but 1e-6 of the rotated offset"""
    with mp().workdps(60):
        rr = _v(r)
        n = _norm(rr)
        d = _cross(rr, [_m(0.3), _m(-0.5), _m(0.8)])
        nd = _norm(d)
        g = [rr[i] + d[i] / nd * (2 * rel * n) for i in range(3)]
        o = _rot(_v(x[3:7]), g)
        return np.array([float(_m(x[i]) + o[i]) for i in range(3)])


@functools.lru_cache(maxsize=None)
def bearing_table(orient, seed=2028):
    """bearing_h<PoseM> with to_point true and false (orient = False), bearing_h<OrientM> (orient = True)"""
    rng = np.random.default_rng(seed + int(orient))
    rows, reg, tp, mounts, points, states = [], [], [], [], [], []

    def add(x, to_point, r, qs, b, name):
        q = x[0:4] if orient else x[3:7]
        r = r if to_point else np.zeros(3)            # the kernel neutralises the lever arm of the direction models
        rows.append(_record(x, q, 1.0 if to_point else 0.0, r, qs, b))
        reg.append(BEARING_REGIMES.index(name))
        tp.append(to_point)
        mounts.append(np.concatenate([r, qs]))
        points.append(b)
        states.append(x)

    state = _orient_state if orient else _pose_state
    for to_point in ((False,) if orient else (True, False)):
        for lever, qs in _mounts(rng):
            for rg in RANGES:
                x = state(rng, 1.0)
                d = rg * _axes(rng, 1)[0]
                add(x, to_point, lever, qs, x[0:3] + d if to_point else d, f"{rg:g}")
            if to_point and np.any(lever != 0):
                x = state(rng, 1.0)
                add(x, True, lever, qs, _cancel_point(x, lever, 1e-6), "cancel")
        # the flag: d = 0 exactly, |d|^2 overflowing, a NaN state entry
        lever, qs = _mounts(rng)[2]
        x = state(rng, 1.0)
        add(x, to_point, np.zeros(3), qs, x[0:3].copy() if to_point else np.zeros(3), "flag")
        add(state(rng, 1.0), to_point, np.zeros(3), qs, np.array([1e200, 0.0, 0.0]), "flag")
        for k in ((0, 3, 6) if to_point else ((0, 3) if orient else (3, 6))):
            x = state(rng, 1.0)
            x[k] = np.nan
            add(x, to_point, lever, qs, x[0:3] + 5.0 if to_point else np.array([0.0, 3.0, 4.0]), "flag")
    return Table(np.array(rows), reg, BEARING_REGIMES, to_point=np.array(tp), mount=np.array(mounts), point=np.array(points),
                 state=np.array(states), orient=orient)


def bearing_reference(tb):
    """(hi, lo, unit [n, 1], recip [n]); the flag records: NaN (only the flag is asserted)"""
    vals, unit = [], []
    nan = mp().mpf("nan")
    flag = BEARING_REGIMES.index("flag")
    with mp().workdps(60):
        for i in range(len(tb.X)):
            if tb.reg[i] == flag:
                vals.append([nan] * 3)
                unit.append(1.0)
                continue
            x, mt, b = tb.raw.state[i], _v(tb.raw.mount[i]), _v(tb.raw.point[i])
            q = _v(x[0:4] if tb.raw.orient else x[3:7])
            v = [b[k] - _m(x[k]) for k in range(3)] if tb.raw.to_point[i] else b
            g = _rot_t(q, v)
            d = _rot_t(mt[3:7], [g[k] - mt[k] for k in range(3)])
            n = _norm(d)
            vals.append([a / n for a in d])
            unit.append(float((_norm(v) + _norm(mt[0:3])) / n))
    hi, lo = _pairs(vals, len(tb.X))
    return hi, lo, np.array(unit)[:, None], np.ones(len(tb.X))


@functools.lru_cache(maxsize=None)
def sensor_table(orient, seed=2029):
    """sensor_h for PoseM (ids 0 ... 4) or OrientM (ids 5 ... 7): one regime and one class per model id"""
    rng = np.random.default_rng(seed + int(orient))
    ids = (5, 6, 7) if orient else (0, 1, 2, 3, 4)
    rows, reg, mounts, points, states, gyros = [], [], [], [], [], []

    def add(mid, x, r, qs, b, gy):
        r = r if mid in READS_LEVER else np.zeros(3)                           # the kernels' neutral inputs
        qs = qs if mid in READS_ROTATION else np.array([0.0, 0.0, 0.0, 1.0])
        b = b if mid in READS_POINT else np.zeros(3)
        rows.append(_record(x, x[0:4] if orient else x[3:7], float(mid), r, qs, b, gy))
        reg.append(mid - ids[0])
        mounts.append(np.concatenate([r, qs]))
        points.append(b)
        states.append(x)
        gyros.append(gy)

    for mid in ids:
        for lever, qs in _mounts(rng):
            for rate in (1.0, 1e-6):
                for rg in RANGES:
                    x = (_orient_state if orient else _pose_state)(rng, rate)
                    d = rg * _axes(rng, 1)[0]
                    add(mid, x, lever, qs, d if orient else x[0:3] + d, rate * rng.normal(size=3))
            if mid == 2 and np.any(lever != 0):
                x = _pose_state(rng, 1.0)
                add(mid, x, lever, qs, _cancel_point(x, lever, 1e-6), np.zeros(3))
    return Table(np.array(rows), reg, [SENSOR_NAMES[i] for i in ids], ids=np.array(reg) + ids[0], mount=np.array(mounts),
                 point=np.array(points), state=np.array(states), gyro=np.array(gyros), orient=orient)


def sensor_reference(tb):
    """(hi, lo, unit [n, 1], recip [n])"""
    vals, unit = [], []
    zero = mp().mpf(0)
    with mp().workdps(60):
        for i in range(len(tb.X)):
            mid = int(tb.raw.ids[i])
            x, mt, b, gy = _v(tb.raw.state[i]), _v(tb.raw.mount[i]), _v(tb.raw.point[i]), _v(tb.raw.gyro[i])
            r, qs = mt[0:3], mt[3:7]
            if mid <= 4:
                p, q, v, w = x[0:3], x[3:7], x[7:10], x[10:13]
                pb = [p[k] - b[k] for k in range(3)]
                if mid == 0:
                    f = _rot(q, r)
                    z, s = [p[k] + f[k] for k in range(3)], _norm(p) + _norm(r)
                elif mid == 1:
                    f = _rot(q, r)
                    z, s = [_norm([pb[k] + f[k] for k in range(3)]), zero, zero], _norm(pb) + _norm(r)
                elif mid == 2:
                    g = _rot_t(q, [-a for a in pb])
                    z, s = _rot_t(qs, [g[k] - r[k] for k in range(3)]), _norm(pb) + _norm(r)
                elif mid == 3:
                    c = _cross(w, r)
                    z, s = _rot_t(qs, [v[k] + c[k] for k in range(3)]), _norm(v) + _norm(w) * _norm(r)
                else:
                    z, s = _rot(q, v), _norm(v)
            else:
                q, v, bg, ba, g = x[0:4], x[4:7], x[7:10], x[10:13], x[13]
                if mid == 5:
                    c = _cross([gy[k] - bg[k] for k in range(3)], r)
                    i3 = _rot_t(q, v)
                    z, s = _rot_t(qs, [i3[k] + c[k] for k in range(3)]), _norm(v) + (_norm(gy) + _norm(bg)) * _norm(r)
                elif mid == 6:
                    z, s = _rot_t(qs, _rot_t(q, b)), _norm(b)
                else:
                    i3 = _rot_t(q, [zero, zero, g])
                    z, s = [i3[k] + ba[k] for k in range(3)], abs(g) + _norm(ba)
            vals.append(z)
            unit.append(float(s))
    hi, lo = _pairs(vals, len(tb.X))
    return hi, lo, np.array(unit)[:, None], np.zeros(len(tb.X))


# ------------------------------------------------------------------------------------------------ the solves
SOLVE_REGIMES = ("identity", "random", "graded", "illcond")


def _spd(rng, m, kind, prec):
    if kind == 0:
        return np.eye(m)
    G = rng.normal(size=(m, m))
    if kind == 1:
        return G @ G.T + 0.5 * np.eye(m)
    if kind == 2:
        d = 10.0 ** np.linspace(-3.0, 3.0, m) if m > 1 else np.array([1e3])
        A = G @ G.T / m + np.eye(m)
        return d[:, None] * A * d[None, :]                      # diagonal graded 1e-6 ... 1e6
    Qm, _ = np.linalg.qr(G)
    ev = 10.0 ** np.linspace(0.0, -8.0 if prec == F64 else -3.0, m) if m > 1 else np.array([1.0])
    return (Qm * ev) @ Qm.T                                     # condition number 1e8 (double), 1e3 (float)


def _factor(A, T):
    """the kernels' elimination in T: lf unscaled (column k: A[r][k] after step k), rs the reciprocal roots of the pivots"""
    m = A.shape[0]
    A = A.astype(T).copy()
    lf, rs = np.full(21, np.nan), np.full(6, np.nan)
    for k in range(m):
        rs[k] = T(1) / np.sqrt(A[k, k])
        for r in range(k, m):
            lf[r * (r + 1) // 2 + k] = A[r, k]
        col = (A[:, k] * T(rs[k])).astype(T)
        for r in range(k + 1, m):
            for c in range(k + 1, r + 1):
                A[r, c] = A[r, c] - col[r] * col[c]
                A[c, r] = A[r, c]
    return lf.astype(T).astype(np.float64), rs.astype(T).astype(np.float64)


@functools.lru_cache(maxsize=None)
def solve_table(prim, prec, m, seed=2030):
    """sampled_solve6 at dimension m (beyond m: lf and rs NaN, c sentinels), or sensor_solve3 (m = 3; the scaled entries l_rk)"""
    T = DT[prec]
    rng = np.random.default_rng(seed + 10 * m + prec)
    rows, reg = [], []
    for kind in range(4):
        for _ in range(1 if kind == 0 else 6):
            lf, rs = _factor(_spd(rng, m, kind, prec), T)
            for scale in (1.0, 1e-3):
                c = (scale * rng.normal(size=m)).astype(T).astype(np.float64)
                r = np.zeros(IN)
                if prim == "solve3":
                    r[0:3], r[6:9] = c, rs[:3]
                    r[3:6] = [float(T(lf[1]) * T(rs[0])), float(T(lf[3]) * T(rs[0])), float(T(lf[4]) * T(rs[1]))]
                else:
                    r[0:6] = SENTINEL + np.arange(6)
                    r[0:m], r[6:27], r[27:33] = c, lf, rs
                rows.append(r)
                reg.append(kind)
    return Table(np.array(rows), reg, SOLVE_REGIMES, m=m, prim=prim)


def solve_factor(tb, r):
    """(Ls as nested lists of mp values, c) of a record"""
    m = tb.raw.m
    if tb.raw.prim == "solve3":
        L = [[1 / _m(r[6]), 0, 0], [_m(r[3]), 1 / _m(r[7]), 0], [_m(r[4]), _m(r[5]), 1 / _m(r[8])]]
    else:
        L = [[(_m(r[6 + i * (i + 1) // 2 + k]) * _m(r[27 + k]) if k < i else (1 / _m(r[27 + k]) if k == i else 0)) for k in range(m)]
             for i in range(m)]
    return L, _v(r[0:m])


def solve_reference(tb):
    """(hi, lo, unit [n, m], recip [n]); unit = |Ls^-1| |Ls| |y|, componentwise"""
    m = tb.raw.m
    vals, unit = [], []
    with mp().workdps(60):
        for r in tb.X:
            L, c = solve_factor(tb, r)
            Lm = mp().matrix(L)
            Li = Lm ** -1
            y = Li * mp().matrix(c)
            absL = mp().matrix(m, m)
            absLi = mp().matrix(m, m)
            for i in range(m):
                for k in range(m):
                    absL[i, k], absLi[i, k] = abs(Lm[i, k]), abs(Li[i, k])
            s = absLi * (absL * mp().matrix([abs(y[k]) for k in range(m)]))
            vals.append([y[k] for k in range(m)])
            unit.append([float(s[k]) for k in range(m)])
    hi, lo = _pairs(vals, len(tb.X))
    return hi, lo, np.array(unit), np.zeros(len(tb.X))


def np_solve(tb, T):
    """the forward substitution in T, as plain NumPy: c[k] = (c[k] - sum_j (lf[k][j] rs[j]) c[j]) rs[k]; -> [n, OUT]"""
    m = tb.raw.m
    X = tb.X.astype(T)
    Y = X[:, 0:OUT].copy()
    if tb.raw.prim == "solve3":
        Y[:, 3:] = 0
        Y[:, 0] = X[:, 0] * X[:, 6]
        Y[:, 1] = (X[:, 1] - X[:, 3] * Y[:, 0]) * X[:, 7]
        Y[:, 2] = ((X[:, 2] - X[:, 4] * Y[:, 0]) - X[:, 5] * Y[:, 1]) * X[:, 8]
        return Y.astype(np.float64)
    for k in range(m):
        v = X[:, k].copy()
        for j in range(k):
            v = v - (X[:, 6 + k * (k + 1) // 2 + j] * X[:, 27 + j]) * Y[:, j]
        Y[:, k] = v * X[:, 27 + k]
    return Y.astype(np.float64)


# ------------------------------------------------------------------------------------------------ tables, references, errors
CASES = ([("s2_log", F64, 0), ("s2_exp", F64, 0)] + [("cos_sinc_sqrt", p, 0) for p in (F64, F32)]
         + [("bearing_pose", F64, 0), ("bearing_orient", F64, 0), ("sensor_pose", F64, 0), ("sensor_orient", F64, 0)]
         + [("solve3", p, 3) for p in (F64, F32)] + [("solve6", p, m) for p in (F64, F32) for m in range(1, 7)])


def case_id(case):
    prim, prec, m = case
    return prim + (f"_m{m}" if prim == "solve6" else "") + ("-f64" if prec == F64 else "-f32")


def table(case):
    prim, prec, m = case
    if prim == "s2_log":
        return log_table()
    if prim == "s2_exp":
        return exp_table()
    if prim == "cos_sinc_sqrt":
        return cos_sinc_table(prec)
    if prim in ("bearing_pose", "bearing_orient"):
        return bearing_table(prim == "bearing_orient")
    if prim in ("sensor_pose", "sensor_orient"):
        return sensor_table(prim == "sensor_orient")
    return solve_table(prim, prec, m)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(hi, lo, unit, recip[, theta]) of the case's table, 40 digits, computed once per process"""
    prim, tb = case[0], table(case)
    with mp().workdps(40):
        if prim == "s2_log":
            return log_reference(tb)
        if prim == "s2_exp":
            return exp_reference(tb)
        if prim == "cos_sinc_sqrt":
            return cos_sinc_reference(tb)
        if prim in ("bearing_pose", "bearing_orient"):
            return bearing_reference(tb)
        if prim in ("sensor_pose", "sensor_orient"):
            return sensor_reference(tb)
        return solve_reference(tb)


def errors(case, Y):
    """per record: the error of outputs Y [n, OUT] in the case's units of eps(T) (max over its outputs).  A record whose
    reference is NaN (the NaN inputs, the flag records): 0 -- those are held by their contracts; any other non-finite output: inf"""
    prim, prec, _ = case
    ref = reference(case)
    hi, lo, unit = ref[0], ref[1], ref[2]
    k = table(case).raw.m if prim == "solve6" else NOUT[prim]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs((Y[:, :k] - hi[:, :k]) - lo[:, :k])
        e = np.where(d == 0, 0.0, d / (EPS[prec] * unit))
    e = np.where(np.isfinite(Y[:, :k]) & ~np.isnan(e), e, np.inf).max(axis=1)
    return np.where(np.isnan(hi[:, 0]), 0.0, e)


def allowance(case):
    """per record, in the case's units: what one hardware-seeded reciprocal of the device code may add to the bound --
    RECIP eps relative, times the size of the result it scales, over the record's unit (s2_log, s2_exp, bearing_h: once)"""
    prim, prec, _ = case
    ref = reference(case)
    unit, recip = ref[2], ref[3]
    with np.errstate(invalid="ignore"):
        a = RECIP[prec] * recip / unit.max(axis=1)
    return np.where(np.isnan(a), 0.0, a)


def by_regime(case, e):
    tb = table(case)
    return {tb.names[c]: float(e[tb.reg == c].max()) for c in sorted(set(tb.reg.tolist()))}


# ------------------------------------------------------------------------------------------------ the table of maxima and bounds
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "meas_primitives_parity.txt")
FLOOR, FACTOR = 4.0, 4.0


def base_bound(ref_alone):
    """the first term of the bound, in units: four times the reference-alone maximum, at least 4 (written with 3 digits)"""
    return float(f"{max(FACTOR * ref_alone, FLOOR):.3g}")


def parse_table(text):
    """{case id: {regime: (reference-alone maximum, bound, device maximum or NaN)}} from lines `<case id> <regime> a/b/c ...`"""
    ids = {case_id(c) for c in CASES}
    out = {}
    for line in text.splitlines():
        f = line.split()
        if len(f) >= 3 and f[0] in ids:
            out[f[0]] = {r: tuple(float(x) if x != "-" else float("nan") for x in v.split("/")) for r, v in zip(f[1::2], f[2::2])}
    return out


def profile_table():
    with open(PROFILE) as fh:
        return parse_table(fh.read())


def _round_up(v):
    """v rounded up to two significant digits"""
    if v <= 0:
        return 0.0
    q = 10.0 ** (int(np.floor(np.log10(v))) - 1)
    return float(f"{np.ceil(v / q - 1e-9) * q:.2g}")


def format_table(ref_alone, device=None):
    """the lines of the table from {case id: {regime: maximum}} of the NumPy statements (CPU) and of the device (or None)"""
    lines = []
    for c in CASES:
        cid = case_id(c)
        cells = []
        for r, v in ref_alone[cid].items():
            listed = _round_up(1.05 * v)          # two digits, 5 % to spare for another libm or SIMD path of NumPy
            dev = "-" if device is None else f"{device[cid][r]:.3g}"
            cells.append(f"{r} {listed:g}/{base_bound(listed):g}/{dev}")
        lines.append(f"{cid:20s} " + "  ".join(f"{x:34s}" for x in cells).rstrip())
    return "\n".join(lines)


def record_bounds(case, listed):
    """per record, in the case's units: the regime's first term (listed: parse_table's dict) plus the reciprocal's allowance"""
    tb = table(case)
    row = listed[case_id(case)]
    return np.array([row[tb.names[c]][1] for c in tb.reg]) + allowance(case)


def roundtrip_bounds(listed):
    """per record of the logarithm's table, in eps, absolute: the bound of s2_exp (its widest regime) plus the record's bound of
    s2_log -- what |s2_exp(u, s2_log(u, v)) - v| is held to"""
    lg, ex = CASES[0], CASES[1]
    return (max(v[1] for v in listed[case_id(ex)].values()) + RECIP[F64]) + record_bounds(lg, listed) * reference(lg)[2][:, 0]


def log_contract_values(Y):
    """of outputs Y of the logarithm's table, per record: the radial share |u.w| / |w| in eps (0 at w = 0) and | |w| - theta_ref |
    in eps, absolute; formed in extended precision.  NaN for the NaN records."""
    tb = log_table()
    u, w = tb.X[:, 0:3].astype(np.longdouble), Y[:, 0:3].astype(np.longdouble)
    nw = np.sqrt(np.sum(w * w, axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        radial = np.where(nw > 0, np.abs(np.sum(u * w, axis=1)) / (EPS[F64] * nw), nw)
        length = np.abs(nw - reference(CASES[0])[4]) / EPS[F64]
    return radial.astype(np.float64), length.astype(np.float64)


# ------------------------------------------------------------------------------------------------ the NumPy statements
def numpy_statement(case):
    """outputs [n, OUT] of the plain NumPy statement of the case's primitive on its table (what the parity tests rely on)"""
    import bearing_reference as br
    import sensor_meas_reference as sr
    prim, prec, _ = case
    tb, T = table(case), DT[prec]
    Y = np.zeros((len(tb.X), OUT))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if prim == "s2_log":
            Y[:, :3] = br.s2_log(tb.X[:, 0:3], tb.X[:, 3:6])
        elif prim == "s2_exp":
            Y[:, :3] = br.s2_exp(tb.X[:, 0:3], tb.X[:, 3:6])
        elif prim == "cos_sinc_sqrt":
            c, s = np_cos_sinc_sqrt(tb.X[:, 0], T)
            Y[:, 0], Y[:, 1] = c, s
        elif prim in ("bearing_pose", "bearing_orient"):
            for i in range(len(tb.X)):
                mid = br.ORIENT_NAV_DIRECTION if tb.raw.orient else (br.POSE_POINT if tb.raw.to_point[i] else br.POSE_NAV_DIRECTION)
                d = br.direction(mid, tb.raw.state[i], tb.raw.mount[i], tb.raw.point[i])
                n2 = float(np.dot(d, d))
                Y[i, :3] = d / np.sqrt(n2)
                Y[i, 3] = 1.0 if (np.isfinite(n2) and n2 > 0) else 0.0
        elif prim in ("sensor_pose", "sensor_orient"):
            for i in range(len(tb.X)):
                z = sr.h(int(tb.raw.ids[i]), tb.raw.state[i], tb.raw.mount[i], tb.raw.point[i], tb.raw.gyro[i])
                Y[i, :len(z)] = z
        else:
            Y = np_solve(tb, T)
    return Y
