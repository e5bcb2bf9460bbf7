"""The device SO(3) primitives of slam-pose_estimation_amd/csrc/ukf_device.hpp, one at a time, against 40-digit references.

tests/cpp/so3_probe.hip includes the shipped header and evaluates one record per lane (fast_rcp, fast_rsqrt, cos_sinc_fast,
so3_exp_fast, so3_exp, so3_log, so3_log_fast, so3_log_fast_n, so3_log_fast_n2, so3_rebase_small, quat_mul, quat_rotate) in
fp64 and fp32.  The inputs sit where these functions switch: the polynomial ranges Y_SMALL / 4 Y_SMALL / U_SMALL and MTK's
taylor_n_bound +- a few ulp, the Cody-Waite ties x = (2k+1) pi, w = +-0 and tiny w (the sign of the plus/minus-periodic log),
+-identity, non-unit quaternions, q = (0, 0, 0, -1) where w + |q| = 0.  The references are mpmath at 40 digits from the
exact binary inputs; the logarithms follow MTK / the oracle: 2 atan(|v| / w) / |v| v with |v| clamped at mtk_tol, and
atan(|v| / +-0) = +-pi/2 as IEEE division gives it.

Errors are in units of eps(T) (2^-52, 2^-23): relative for fast_rcp / fast_rsqrt; absolute for the unit-scale outputs,
divided by max(1, x) where an angle x is reduced modulo 2 pi (cos_sinc: x = sqrt(y); exp: x = |v scale| / 2) because the
rounding of x itself is that large; divided by max(1, |a| |b|) and max(1, |q|^2 |v|) for quat_mul and quat_rotate.
Each bound is at most four times the largest error observed on the MI355X; the docstring of test_primitive_against_40_digits
lists both, per primitive, precision and regime (the regime is the path the lane takes, as the kernel decides it).

Neighbour independence: the wide-angle code runs behind wave-uniform votes, and each lane must keep the result of its own
regime.  Every input is also evaluated in waves of its own regime, with one lane of another regime (or a NaN lane) at the
16-lane row and half-wave boundaries 0, 15, 16, 31, 32, 47, 48, 63, and alternating with another regime; its output bits
must be those of the all-own-regime wave."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from probe_support import DT, EPS, F32, F64, _axes, _m, _ulps, load, placements  # noqa: E402

IN, OUT = 12, 8                      # doubles per record (tests/cpp/so3_probe.hip SO3P_IN / SO3P_OUT)
PRIM = dict(rcp=0, rsqrt=1, cos_sinc=2, exp_fast=3, exp=4, log=5, log_fast=6, log_fast_n=7, log_fast_n2=8, rebase=9,
            quat_mul=10, quat_rotate=11)
NOUT = dict(rcp=1, rsqrt=1, cos_sinc=2, exp_fast=4, exp=4, log=3, log_fast=3, log_fast_n=3, log_fast_n2=6, rebase=3,
            quat_mul=4, quat_rotate=3)
Y_SMALL = {F64: np.float64(0.62), F32: np.float32(0.62)}
U_SMALL = {F64: np.float64(0.07), F32: np.float32(0.07)}
TAYLOR_N = {F64: np.float64(0.0001220703125), F32: np.float32(0.018581361)}   # Num<T>::taylor_n_bound
MTK_TOL = {F64: 1e-11, F32: float(np.float32(1e-5))}                           # Num<T>::mtk_tol
REGIMES = dict(rcp=("all",), rsqrt=("all",), cos_sinc=("small", "doubled", "reduced"),
               exp_fast=("small", "doubled", "reduced"), exp=("taylor", "sincos"), log=("all",), log_fast=("small", "wide"),
               log_fast_n=("small", "wide"), log_fast_n2=("ss", "sw", "ws", "ww"), rebase=("all",), quat_mul=("all",),
               quat_rotate=("all",))

def _bounds(table):
    """{(prim, prec): {regime: (observed, bound)}} from the docstring table of test_primitive_against_40_digits"""
    out = {}
    for line in table.splitlines():
        f = line.split()
        if len(f) < 3 or f[0] not in PRIM or f[1] not in ("f64", "f32"):
            continue
        out[(f[0], F64 if f[1] == "f64" else F32)] = {
            r: (float(v.split("/")[0]), float(v.split("/")[1])) for r, v in zip(f[2::2], f[3::2])}
    return out


# ------------------------------------------------------------------------------------------------ 40-digit references
def ref_exp(v, scale):
    """MTK SO3::exp(v, scale): (sinc(a) (scale/2) v, cos a), a = |v| |scale| / 2 (storage x y z w)"""
    v = [_m(c) for c in v]
    h = _m(scale) / 2
    a = mp.sqrt(sum(c * c for c in v)) * h
    sinc = mp.sin(a) / a if a != 0 else mp.mpf(1)
    return [sinc * h * c for c in v] + [mp.cos(a)]


def ref_log(q, tol):
    """MTK SO3::log = the oracle's so3_log: 2 atan(nv / w) / nv * v, nv = max(|v|, tol), plus/minus periodic;
    nv / +-0 is +-inf, whose atan is +-pi/2"""
    x, y, z, w = (_m(c) for c in q)
    nv = mp.sqrt(x * x + y * y + z * z)
    if nv < tol:
        nv = _m(tol)
    at = mp.atan(nv / w) if w != 0 else math.copysign(1.0, float(q[3])) * mp.pi / 2
    s = 2 * at / nv
    return [s * x, s * y, s * z]


def ref_qmul(a, b):
    ax, ay, az, aw = (_m(c) for c in a)
    bx, by, bz, bw = (_m(c) for c in b)
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]


def ref_rotate(q, v):
    """Eigen _transformVector: v + 2 w (vec x v) + 2 vec x (vec x v), also for non-unit q"""
    qv, w, v = [_m(c) for c in q[:3]], _m(q[3]), [_m(c) for c in v]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    u = cross(qv, v)
    c = cross(qv, u)
    return [v[k] + 2 * (w * u[k] + c[k]) for k in range(3)]


def ref_rebase(d, a):
    """log(exp(-a) exp(d)) exactly (angles below pi: the plain log)"""
    return ref_log(ref_qmul(ref_exp([-_m(c) for c in a], 1), ref_exp(d, 1)), 0)


def _reference(prim, prec, r):
    tol = MTK_TOL[prec]
    if prim == "rcp":
        return [1 / _m(r[0])]
    if prim == "rsqrt":
        return [1 / mp.sqrt(_m(r[0]))]
    if prim == "cos_sinc":
        y = _m(r[0])
        x = mp.sqrt(y)
        return [mp.cos(x), mp.sin(x) / x if y != 0 else mp.mpf(1)]
    if prim in ("exp_fast", "exp"):
        return ref_exp(r[:3], r[3])
    if prim in ("log", "log_fast", "log_fast_n"):
        return ref_log(r[:4], tol)
    if prim == "log_fast_n2":
        return ref_log(r[:4], tol) + ref_log(r[4:8], tol)
    if prim == "rebase":
        return ref_rebase(r[:3], r[3:6])
    if prim == "quat_mul":
        return ref_qmul(r[:4], r[4:8])
    if prim == "quat_rotate":
        return ref_rotate(r[:4], r[4:7])
    raise KeyError(prim)


def reference(prim, prec, X):
    """(hi, lo) double-double of the 40-digit reference of every record"""
    hi = np.zeros((X.shape[0], OUT))
    lo = np.zeros((X.shape[0], OUT))
    with mp.workdps(40):
        for i, r in enumerate(X):
            for k, v in enumerate(_reference(prim, prec, r)):
                h = float(v)
                hi[i, k], lo[i, k] = h, float(v - h)
    return hi, lo


# ------------------------------------------------------------------------------------------------ inputs at the edges
def _rec(rows):
    X = np.zeros((len(rows), IN))
    for i, r in enumerate(rows):
        X[i, :len(r)] = r
    return X


def _quat(axis, theta):
    return np.concatenate([np.sin(theta / 2) * axis, [np.cos(theta / 2)]])


def _log_quats(rng, prec, m):
    """quaternions for the logarithms: angles over (0, 2 pi) (both signs of w), w near and at +-0, +-identity, tiny |v|,
    |v|^2 / w^2 = U_SMALL +- k ulp, non-unit norms"""
    T = DT[prec]
    ax = _axes(rng, m)
    th = rng.uniform(0.0, 2 * np.pi, m)
    qs = [_quat(ax[i], th[i]) for i in range(m)]
    for w in (1e-8, -1e-8, 1e-17, -1e-17, 0.0, -0.0):
        for a in _axes(rng, 3):
            s = math.sqrt(1.0 - w * w)
            qs.append(np.array([s * a[0], s * a[1], s * a[2], w]))
    qs += [np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.0, -1.0])]
    for a in _axes(rng, 2):
        qs += [np.concatenate([1e-20 * a, [1.0]]), np.concatenate([1e-20 * a, [-1.0]])]
    for t in _ulps(math.sqrt(float(U_SMALL[prec])), 4, T):
        qs += [np.array([float(t), 0.0, 0.0, 1.0]), np.array([0.0, float(t), 0.0, -1.0])]
    base = list(qs[:m // 4])
    for s in (0.5, 1.01, 2.0):
        qs += [s * q for q in base[: m // 12]]
    return [np.asarray(q, dtype=T).astype(np.float64) for q in qs]


def _norm_T(q, T):
    with mp.workdps(40):
        return float(T(float(mp.sqrt(sum(_m(c) ** 2 for c in q)))))


def inputs(prim, prec, seed=2024):
    """records (m x IN, exact in T) and the regime of every record (index into REGIMES[prim])"""
    T = DT[prec]
    rng = np.random.default_rng(seed + 17 * PRIM[prim] + prec)
    ys, ysm = Y_SMALL[prec], T(4) * Y_SMALL[prec]
    if prim in ("rcp", "rsqrt"):
        xs = list(10.0 ** rng.uniform(-30, 30, 1200))
        for e in range(-99, 100, 3):
            xs += _ulps(2.0 ** e, 1, T)
        xs = np.asarray(xs, dtype=T).astype(np.float64)
        if prim == "rcp":
            xs = np.concatenate([xs, -xs[::3]])
        X = _rec([[x] for x in xs])
        return X, np.zeros(len(X), dtype=int)
    if prim == "cos_sinc":
        ys_ = [0.0, 1e-30, 1e-20, 1e-12, 1e-6]
        for e in (ys, ysm):
            ys_ += _ulps(e, 4, T)
        ys_ += [(np.pi / 2) ** 2, np.pi ** 2]
        for k in range(1, 301):
            ys_ += [(2 * np.pi * k) ** 2, ((2 * k + 1) * np.pi) ** 2]
        ys_ += list((10.0 ** rng.uniform(-4, 3, 1500)) ** 2)
        y = np.asarray(ys_, dtype=T)
        cls = np.where(y <= ys, 0, np.where(y <= ysm, 1, 2))
        return _rec([[v] for v in y.astype(np.float64)]), cls
    if prim in ("exp_fast", "exp"):
        m = 1500
        ax = _axes(rng, m)
        ang = 10.0 ** rng.uniform(-8, np.log10(60.0), m)              # |v scale|
        scale = rng.choice([1.0, 0.01, 0.1, -1.0, -0.01], m)
        rows = [list(ax[i] * ang[i] / abs(scale[i])) + [scale[i]] for i in range(m)]
        # switch points: v = (x, 0, 0), scale 2 -> the argument of cos_sinc is x^2
        for e in (ys, ysm, TAYLOR_N[prec]):
            for x in _ulps(math.sqrt(float(e)), 4, T):
                rows += [[float(x), 0.0, 0.0, 2.0], [0.0, 0.0, -float(x), -2.0]]
        rows += [[0.0, 0.0, 0.0, 1.0], [np.pi, 0.0, 0.0, 1.0], [0.0, 2 * np.pi, 0.0, 1.0], [0.0, 0.0, 7.0, 1.0]]
        X = _rec(rows).astype(T).astype(np.float64)
        v, s = X[:, :3].astype(T), X[:, 3].astype(T)
        yy = (s * T(0.5)) * (s * T(0.5)) * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        if prim == "exp":
            cls = (yy >= TAYLOR_N[prec]).astype(int)
        else:
            cls = np.where(yy <= ys, 0, np.where(yy <= ysm, 1, 2))
        return X, cls
    if prim in ("log", "log_fast", "log_fast_n"):
        qs = _log_quats(rng, prec, 1500)
        if prim == "log_fast_n":
            # tan^2(phi/2) = |v|^2 / (w + |q|)^2 = U_SMALL +- k ulp, and w + |q| = 0
            t0 = 2 * math.sqrt(float(U_SMALL[prec])) / (1 - float(U_SMALL[prec]))   # |v| / w of a unit quaternion at the edge
            for t in _ulps(t0, 4, T):
                qs.append(np.asarray([float(t), 0.0, 0.0, 1.0], dtype=T).astype(np.float64))
            qs.append(np.array([0.0, 0.0, 0.0, -1.0]))
        rows = [list(q) + ([_norm_T(q, T)] if prim == "log_fast_n" else []) for q in qs]
        X = _rec(rows)
        q = X[:, :4].astype(T)
        v2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]
        with np.errstate(all="ignore"):
            if prim == "log_fast":
                u = v2 / (q[:, 3] * q[:, 3])
            else:
                u = v2 / ((q[:, 3] + X[:, 4].astype(T)) ** 2)
        cls = np.zeros(len(X), dtype=int) if prim == "log" else (~(u <= U_SMALL[prec])).astype(int)
        return X, cls
    if prim == "log_fast_n2":
        rows, cls = [], []
        m = 300
        for ca in (0, 1):
            for cb in (0, 1):
                for i in range(m):
                    s = rng.choice([1.0, 1.0, 0.5, 1.01, 2.0])
                    th = [rng.uniform(0.0, 1.0) if c == 0 else rng.uniform(1.2, 2 * np.pi) for c in (ca, cb)]
                    ax = _axes(rng, 2)
                    qa = np.asarray(s * _quat(ax[0], th[0]), dtype=T).astype(np.float64)
                    qb = np.asarray(s * _quat(ax[1], th[1]), dtype=T).astype(np.float64)
                    rows.append(list(qa) + list(qb) + [_norm_T(qa, T)])
                    cls.append(2 * ca + cb)
        # signed zeros and q = -1 against a small partner, both ways
        small = np.array([0.01, -0.02, 0.03, math.sqrt(1 - 0.0014)])
        for wide in (np.array([0.6, 0.0, 0.8, 0.0]), np.array([0.6, 0.0, 0.8, -0.0]), np.array([0.0, 0.0, 0.0, -1.0])):
            rows.append(list(small) + list(wide) + [1.0]); cls.append(1)
            rows.append(list(wide) + list(small) + [1.0]); cls.append(2)
        X = _rec(rows)
        X[:, :9] = X[:, :9].astype(T).astype(np.float64)
        return X, np.asarray(cls)
    if prim == "rebase":
        m = 1500
        d = _axes(rng, m) * np.sqrt(rng.uniform(0.0, 2.25, m))[:, None]
        a = _axes(rng, m) * np.sqrt(10.0 ** rng.uniform(-24, -12, m))[:, None]
        d, a = d.astype(T), a.astype(T)
        a2 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]
        X = _rec([list(d[i]) + list(a[i]) + [a2[i]] for i in range(m)])
        return X, np.zeros(m, dtype=int)
    if prim in ("quat_mul", "quat_rotate"):
        m = 1000
        qa = rng.normal(size=(m, 4)) * rng.uniform(0.5, 2.0, (m, 1)) / 2
        qb = rng.normal(size=(m, 4 if prim == "quat_mul" else 3))
        X = _rec([list(qa[i]) + list(qb[i]) for i in range(m)]).astype(T).astype(np.float64)
        return X, np.zeros(m, dtype=int)
    raise KeyError(prim)


def _scale(prim, X):
    """the normalisation of every record's absolute error (module docstring)"""
    one = np.ones(X.shape[0])
    if prim == "cos_sinc":
        return np.maximum(one, np.sqrt(X[:, 0]))
    if prim in ("exp_fast", "exp"):
        return np.maximum(one, np.linalg.norm(X[:, :3], axis=1) * np.abs(X[:, 3]) / 2)
    if prim == "quat_mul":
        return np.maximum(one, np.linalg.norm(X[:, :4], axis=1) * np.linalg.norm(X[:, 4:8], axis=1))
    if prim == "quat_rotate":
        return np.maximum(one, np.linalg.norm(X[:, :4], axis=1) ** 2 * np.linalg.norm(X[:, 4:7], axis=1))
    return one


# ------------------------------------------------------------------------------------------------ the device
def _lib():
    return load("libso3_probe", so3_probe=(C.c_int, (C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double))))


def device(prim, prec, X):
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.zeros((X.shape[0], OUT))
    rc = _lib().so3_probe(PRIM[prim], prec, X.shape[0], X.ctypes.data_as(C.POINTER(C.c_double)),
                          Y.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, rc
    return Y


@functools.lru_cache(maxsize=None)
def evaluate(prim, prec):
    """inputs, regimes, device outputs in the all-own-regime waves, and whether every placement gave the same bits"""
    X, cls = inputs(prim, prec)
    src, base = placements(cls)
    Xs = np.where(src[:, None] >= 0, X[np.maximum(src, 0)], np.nan)
    Y = device(prim, prec, Xs)
    Yb = Y[base]
    bits = Y.view(np.int64)
    ok = src >= 0
    moved = np.nonzero(ok & np.any(bits != Yb.view(np.int64)[np.maximum(src, 0)], axis=1))[0]
    return X, cls, Yb, src[moved], Y[moved]


@functools.lru_cache(maxsize=None)
def errors(prim, prec):
    """per record: the normalised error in eps(T) (max over its outputs)"""
    X, cls, Yb, _, _ = evaluate(prim, prec)
    hi, lo = reference(prim, prec, X)
    k = NOUT[prim]
    d = np.abs((Yb[:, :k] - hi[:, :k]) - lo[:, :k])
    if prim in ("rcp", "rsqrt"):
        d = d / np.abs(hi[:, :k])
    e = np.max(d, axis=1) / _scale(prim, X) / EPS[prec]
    return np.where(np.isnan(e), np.inf, e)


def observed():
    """{(prim, prec): {regime: max error}}: the observed column of the bounds table (re-measure after a kernel change)"""
    out = {}
    for prim in PRIM:
        for prec in (F64, F32):
            X, cls, _, _, _ = evaluate(prim, prec)
            e = errors(prim, prec)
            out[(prim, prec)] = {REGIMES[prim][c]: float(e[cls == c].max()) for c in sorted(set(cls.tolist()))}
    return out


CASES = [(p, q) for p in PRIM for q in (F64, F32)]
IDS = [f"{p}-{'f64' if q == F64 else 'f32'}" for p, q in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("prim,prec", CASES, ids=IDS)
def test_primitive_against_40_digits(prim, prec):
    """Largest error observed on the MI355X / bound, in eps(T) as the module docstring normalises it, per regime:

    rcp          f64  all 9.51/24
    rcp          f32  all 0.685/2
    rsqrt        f64  all 8.45/24
    rsqrt        f32  all 0.669/2
    cos_sinc     f64  small 0.682/2     doubled 2.50/8    reduced 11.8/32
    cos_sinc     f32  small 0.287/1     doubled 1.13/4    reduced 1.70/6
    exp_fast     f64  small 0.688/2     doubled 2.22/8    reduced 11.3/32
    exp_fast     f32  small 0.463/1.5   doubled 1.06/4    reduced 1.52/6
    exp          f64  taylor 0.657/2    sincos 0.664/2
    exp          f32  taylor 0.489/1.5  sincos 0.860/3
    log          f64  all 3.51/12
    log          f32  all 4.90/16
    log_fast     f64  small 0.746/2     wide 9.33/32
    log_fast     f32  small 0.432/1.5   wide 5.07/16
    log_fast_n   f64  small 2.30/8      wide 8.93/32
    log_fast_n   f32  small 0.970/3     wide 5.58/16
    log_fast_n2  f64  ss 2.82/8         sw 12.3/40        ws 7.02/24        ww 10.4/32
    log_fast_n2  f32  ss 1.17/4         sw 4.58/16        ws 4.76/16        ww 4.88/16
    rebase       f64  all 114/256
    rebase       f32  all 1.33/4
    quat_mul     f64  all 1.03/4
    quat_mul     f32  all 0.839/3
    quat_rotate  f64  all 1.67/6
    quat_rotate  f32  all 1.91/6

    (so3_log_fast_n2: the sw / ws columns are the pairs with one small and one wide logarithm; rebase f64: the series
    remainder, below 4e-14 = 180 eps by construction, dominates.)"""
    X, cls, Yb, _, _ = evaluate(prim, prec)
    e = errors(prim, prec)
    assert set(cls.tolist()) == set(range(len(REGIMES[prim]))), "every regime has inputs"
    worst = {}
    for c, name in enumerate(REGIMES[prim]):
        sel = cls == c
        i = int(np.argmax(np.where(sel, e, -1.0)))
        worst[name] = (float(e[i]), X[i, :9].tolist(), Yb[i, :NOUT[prim]].tolist())
        assert e[i] <= BOUNDS[(prim, prec)][name][1], (name, worst[name])


BOUNDS = _bounds(test_primitive_against_40_digits.__doc__)


@pytest.mark.gpu
@pytest.mark.parametrize("prim,prec", CASES, ids=IDS)
def test_neighbour_independence(prim, prec):
    """bit-exact: a lane's result does not depend on the regime (or NaN) of the other lanes of its wavefront"""
    X, cls, Yb, moved_src, moved_out = evaluate(prim, prec)
    assert moved_src.size == 0, (moved_src[:4].tolist(), X[moved_src[:4], :9].tolist(), moved_out[:4].tolist(),
                                 Yb[moved_src[:4]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_log_fast_n2_is_two_log_fast_n(prec):
    """so3_log_fast_n2 does the arithmetic of two so3_log_fast_n calls under one vote: bit-identical results (observed on the
    MI355X for every record of every placement, in both precisions)"""
    X, cls, Yb, _, _ = evaluate("log_fast_n2", prec)
    src, base = placements(cls)
    for part in (0, 1):
        Xn = np.zeros_like(X)
        Xn[:, :4], Xn[:, 4] = X[:, 4 * part:4 * part + 4], X[:, 8]
        Yn = device("log_fast_n", prec, np.where(src[:, None] >= 0, Xn[np.maximum(src, 0)], np.nan))[base]
        assert (Yn[:, :3].view(np.int64) == Yb[:, 3 * part:3 * part + 3].view(np.int64)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_log_at_signed_zero_w_follows_mtk(prec):
    """w = -0.0: MTK's atan(|v| / -0) = -pi/2 gives -pi v/|v|; w = +0.0 gives +pi v/|v| (the plus/minus periodic log)"""
    v = np.array([0.6, 0.0, 0.8])
    for w, sign in ((0.0, 1.0), (-0.0, -1.0)):
        q = np.concatenate([v, [w]])
        want = sign * np.pi * v
        for prim, row in (("log", q), ("log_fast", q), ("log_fast_n", np.concatenate([q, [1.0]])),
                          ("log_fast_n2", np.concatenate([q, q, [1.0]]))):
            Y = device(prim, prec, np.resize(_rec([row]), (64, IN)))
            got = Y[0, :NOUT[prim]].reshape(-1, 3)
            assert np.abs(got - want).max() <= 8 * EPS[prec] * np.pi, (prim, w, got.tolist())


# ------------------------------------------------------------------------------------------------ the references on the CPU
def test_references_match_the_oracle(oracle):
    """The semantics the device is held to: ref_exp / ref_log agree with the oracle's so3_exp / so3_log (fp64) across w = 0
    (the plus/minus periodicity), at both signed zeros, at the mtk_tol clamp and at the Taylor switch of exp."""
    rng = np.random.default_rng(3)
    qs = []
    for th in list(rng.uniform(0, 2 * np.pi, 40)) + [np.pi - 1e-9, np.pi, np.pi + 1e-9]:
        qs.append(_quat(_axes(rng, 1)[0], th))
    for w in (1e-8, -1e-8, 1e-17, -1e-17, 0.0, -0.0):
        s = math.sqrt(1 - w * w)
        qs.append(np.array([0.6 * s, 0.0, -0.8 * s, w]))
    qs += [np.array([1e-12, 0.0, 0.0, 1e-12]), np.array([3e-12, -4e-12, 0.0, -2e-12]), np.array([1e-20, 0.0, 0.0, 1.0]),
           np.array([0.0, 0.0, 0.0, -1.0]), np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.3, 0.2, 0.1, -0.5])]
    worst = 0.0
    with mp.workdps(40):
        for q in qs:
            ref = np.array([float(c) for c in ref_log(q, MTK_TOL[F64])])
            got = oracle.so3_log(q)
            assert (np.sign(ref) == np.sign(got)).all(), (q.tolist(), ref.tolist(), got.tolist())
            worst = max(worst, float(np.abs(ref - got).max()))
        # the clamp matters: nv = 1e-12 < mtk_tol with w = 1e-12 is 2 atan(10) / 10 per unit of v, not pi/2
        assert abs(float(ref_log([1e-12, 0.0, 0.0, 1e-12], MTK_TOL[F64])[0]) - 0.2 * math.atan(10.0)) < 1e-15
        assert float(ref_log([0.6, 0.0, 0.8, -0.0], MTK_TOL[F64])[0]) < 0
        x0 = math.sqrt(float(TAYLOR_N[F64]))
        vs = [(x, 2.0) for x in _ulps(x0, 4, np.float64)] + [(a * t, s) for a, t, s in
                                                            zip(_axes(rng, 30), 10.0 ** rng.uniform(-8, 1.5, 30),
                                                                rng.choice([1.0, -1.0, 0.01], 30))]
        for v, s in vs:
            v = np.array([float(v), 0.0, 0.0]) if np.ndim(v) == 0 else v
            ref = np.array([float(c) for c in ref_exp(v, s)])
            worst = max(worst, float(np.abs(ref - oracle.so3_exp(v, s)).max()))
    assert worst <= 2e-15, worst
