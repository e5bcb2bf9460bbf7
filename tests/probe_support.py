"""Support for the tests that drive the device helper libraries of tests/cpp (the SO(3), Jacobian and Cholesky probes, the LDS
poisoner): one loader, and the record plumbing the SO(3) and Jacobian probe tests share.  No tests here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
POS = (0, 15, 16, 31, 32, 47, 48, 63)   # 16-lane DPP rows and half-waves of a 64-lane wavefront
F64, F32 = 0, 1
DT = {F64: np.float64, F32: np.float32}
EPS = {F64: 2.0 ** -52, F32: 2.0 ** -23}
LDS_PATTERNS = (0x7FC00000, 0x7F800000, 0xFFFFFFFF, 0x00000000)     # float NaN, float +Inf, a NaN in both precisions, zero


@functools.lru_cache(maxsize=None)
def load(name, **signatures):
    """tests/cpp/build/<name>.so, built through make when missing; signatures: function=(restype, argtypes), hashable"""
    path = os.path.join(CPP, "build", name + ".so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", CPP, "build/" + name + ".so"])
    lib = C.CDLL(path)
    for fn, (restype, argtypes) in signatures.items():
        getattr(lib, fn).restype = restype
        getattr(lib, fn).argtypes = list(argtypes)
    return lib


def lds_poison():
    """lds_poison(pattern) of tests/cpp/lds_poison.hip: fills the LDS of every CU with a bit pattern; returns 0"""
    return _lds_library().lds_poison


def _lds_library():
    return load("liblds_poison", lds_poison=(C.c_int, (C.c_uint32,)),
                lds_leftovers_seen=(C.c_int, (C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))))


def lds_leftovers_seen():
    """seen(pattern) -> (matched, read) by lds_leftovers_seen of tests/cpp/lds_poison.hip: a kernel of the fill's geometry that
    writes no LDS counts the dwords of its own allocation that still hold the pattern"""
    fn = _lds_library().lds_leftovers_seen

    def seen(pattern):
        matched, read = C.c_uint64(0), C.c_uint64(0)
        rc = fn(pattern, C.byref(matched), C.byref(read))
        assert rc == 0, rc
        return int(matched.value), int(read.value)
    return seen


def _m(x):
    """exact: a double (or a numpy scalar) as it is, an mpf unrounded"""
    import mpmath as mp   # here, so that the loader serves tests that need no mpmath
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


def _ulps(x, k, T):
    """x moved by -k..k ulp of T"""
    x = T(x)
    out = [x]
    up = dn = x
    for _ in range(k):
        up, dn = np.nextafter(up, T(np.inf)), np.nextafter(dn, T(-np.inf))
        out += [up, dn]
    return out


def _axes(rng, m):
    a = rng.normal(size=(m, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def placements(cls):
    """Record order of one launch: every regime in waves of its own (the base position of each record), then each regime's
    records in waves with one lane of another regime or a NaN record (index -1) at each of POS, then regimes alternating."""
    regimes = sorted(set(cls.tolist()))
    ids = {c: np.nonzero(cls == c)[0] for c in regimes}
    src, base, n0 = [], np.empty(len(cls), dtype=np.int64), 0
    for c in regimes:
        base[ids[c]] = n0 + np.arange(len(ids[c]))
        src.append(np.resize(ids[c], -(-len(ids[c]) // 64) * 64))
        n0 += src[-1].size
    for a in regimes:
        nw = -(-len(ids[a]) // 63)
        fill = np.resize(ids[a], nw * 63).reshape(nw, 63)
        for b in [r for r in regimes if r != a] + [None]:
            foreign = np.full(nw, -1) if b is None else np.resize(ids[b], nw)
            for p in POS:
                src.append(np.insert(fill, p, foreign, axis=1).ravel())
    for i, a in enumerate(regimes):
        for b in regimes[i + 1:]:
            k = max(len(ids[a]), len(ids[b]))
            alt = np.stack([np.resize(ids[a], k), np.resize(ids[b], k)], axis=1).ravel()
            src.append(np.resize(alt, -(-alt.size // 64) * 64))
    src = np.concatenate(src)
    assert src.size % 64 == 0 and n0 % 64 == 0
    return src, base
