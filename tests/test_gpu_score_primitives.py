"""The device's scoring primitives of the robust and the relative update -- robust_eval, robust_scale
(slam-pose_estimation_amd/csrc/ukf_robust.hpp), relative_chol6, relative_solve6 (ukf_relative.hpp) -- against 40-digit references
at their regime edges.  The kernels that use them are otherwise checked end to end only: tests/test_gpu_robust.py on cycled engines
with cond(S) <= 2000 and outliers of rho <= 300 against the kernel's own rule restated, tests/test_gpu_relative.py on benign S.

tests/cpp/score_probe.hip includes the shipped headers and evaluates one record per lane; tests/score_primitives_reference.py holds
the case tables, the references, the units, the verdict margins (its docstring) and the assertions themselves, which
tests/test_score_primitives_reference.py applies to the NumPy statements of the same primitives on the same tables.

Bounds.  A record's bound, in its unit of eps(T), is four times the largest error of the NumPy statement in the record's regime
(measured on the CPU, two digits, 5 % to spare, at least 4) plus 24 eps (fp64) / 2 eps (fp32) once per hardware-seeded reciprocal
on the path to the result.  No bound comes from device output; the tests read profiles/score_primitives_parity.txt (reference-alone
maximum / first term of the bound / largest error seen on the MI355X, the last for information).

MATCH.  The returned lambda is judged by its residual in exact arithmetic, r = f_40(lambda) / c^2 - 1 on the T-rounded inputs:
rows that neither clamp nor reach the step cap hold -slack <= r <= tol + slack with slack = (bound of f) eps kappa_H(S(lambda)).
The left inequality is the header's "the iterates never pass the root", up to rounding.  The step count equals the reference's own
where every 40-digit iterate's residual is clear of tol by more than 2 slack (m1, proportional and benign at the loose tolerance:
every record); elsewhere its <= max_iter.  HUBER: the relative error of lambda within half the bound of d0^2 plus 2 eps.

Contracts, bit for bit: lambda == 1 and its == 0 for an inlier, an ineligible, gated or NaN row, a row whose S(1) fails and a row
whose S(1)^-1 nu lies in the null space of Q; lambda == scale_max where the root lies above it; d0sq is robust_eval's f at
lambda = 1; ok is the verdict on every record (each clearly positive definite or clearly not); an identity part of the 6 x 6
matrix gives exact 0 / 1 in L, rs == 1, y == v there and adds exactly 0 to lndet.

Neighbour independence, bit for bit: robust_scale loops under a wave vote with finished rows riding along under selects.  Every
record is evaluated in waves of its own regime, with one lane of another regime (another trip count) or a NaN record at lanes 0,
15, 16, 31, 32, 47, 48, 63, alternating with another regime, and in a launch in table order whose last wavefront is ragged; its
output bits must be those of the first."""
import ctypes as C
import functools

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import score_primitives_reference as sr  # noqa: E402
from probe_support import F32, F64, load, placements  # noqa: E402

_D = C.POINTER(C.c_double)
PREC = [F64, F32]
PREC_IDS = ["f64", "f32"]
BOUND_TAGS = ("f", "g", "L", "lndet", "y", "d2", "huber lambda", "-slack <= r <= tol + slack")


class ScoreRule(C.Structure):
    _fields_ = [("mode", C.c_int), ("max_iter", C.c_int), ("chi2_m1", C.c_double), ("chi2_m3", C.c_double), ("scale_max", C.c_double),
                ("tol", C.c_double), ("gate_chi2", C.c_double)]


def _lib():
    return load("libscore_probe", score_probe=(C.c_int, (C.c_int, C.c_int, C.POINTER(ScoreRule), C.c_int64, _D, _D)))


def device(prim, prec, X, rl=None):
    X = np.ascontiguousarray(X, dtype=np.float64)
    assert X.shape[1] == sr.IN
    Y = np.zeros((X.shape[0], sr.OUT))
    r = None if rl is None else C.byref(ScoreRule(rl.mode, rl.max_iter, rl.chi2_m1, rl.chi2_m3, rl.scale_max, rl.tol, rl.gate_chi2))
    rc = _lib().score_probe(sr.PRIM[prim], prec, r, X.shape[0], X.ctypes.data_as(_D), Y.ctypes.data_as(_D))
    assert rc == 0, rc
    return Y


def _table(prim, prec, case):
    if prim == "eval":
        return sr.eval_table(prec), None
    if prim == "scale":
        return sr.scale_case(prec, case)
    return sr.chol_table(prec), None


@functools.lru_cache(maxsize=None)
def run(prim, prec, case=None):
    """the device outputs of a case's table, in table order"""
    tb, rl = _table(prim, prec, case)
    return device(prim, prec, tb.X, rl)


@functools.lru_cache(maxsize=None)
def listed():
    return sr.profile_table()


def _report(name, maxima):
    for k, v in maxima.items():
        print(f"PARITY score {name} {k}: " + (", ".join(f"{r} {x:.3g}" for r, x in v.items()) if isinstance(v, dict) else str(v)))


def _split(fails, bounds):
    return [f for f in fails if (f[0] in BOUND_TAGS) == bounds]


@functools.lru_cache(maxsize=None)
def _eval(prec):
    return sr.eval_failures(prec, run("eval", prec), listed())


@functools.lru_cache(maxsize=None)
def _scale(prec, case):
    return sr.scale_failures(prec, case, run("scale", prec, case), listed())


@functools.lru_cache(maxsize=None)
def _chol(prec):
    return sr.chol_failures(prec, run("chol6", prec), run("solve", prec), listed())


def observed():
    """{line id: {regime: max error}} of the device: the third column of the table (re-measure after a kernel change)"""
    out = {}
    for prec, p in sr.PRECS:
        out.update(_eval(prec)[0])
        out.update(_chol(prec)[0])
        for t in sr.SCALE_TABLES:
            acc = {}
            for case, (tname, _) in sr.SCALE_CASES.items():
                if tname == t:
                    acc = sr.merge_max(acc, _scale(prec, case)[0])
            out[f"scale_{t}_f-{p}"] = acc
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("bounds", [True, False], ids=["bounds", "contracts"])
@pytest.mark.parametrize("prec", PREC, ids=PREC_IDS)
def test_robust_eval(prec, bounds):
    """f and g of every record within their bounds; ok is the verdict; NaN in, NaN out"""
    maxima, fails = _eval(prec)
    _report("eval", maxima)
    assert not _split(fails, bounds), _split(fails, bounds)


@pytest.mark.gpu
@pytest.mark.parametrize("bounds", [True, False], ids=["bounds", "contracts"])
@pytest.mark.parametrize("case", list(sr.SCALE_CASES))
@pytest.mark.parametrize("prec", PREC, ids=PREC_IDS)
def test_robust_scale(prec, case, bounds):
    """bounds: d0sq and f at the returned lambda, the MATCH residual, HUBER's lambda.  contracts: the module docstring's"""
    maxima, lines, fails = _scale(prec, case)
    _report(f"scale {case} {sr.PRECS[prec][1]} f", {"device": maxima})
    _report(f"scale {case} {sr.PRECS[prec][1]}", dict(lines))
    assert not _split(fails, bounds), _split(fails, bounds)


@pytest.mark.gpu
@pytest.mark.parametrize("bounds", [True, False], ids=["bounds", "contracts"])
@pytest.mark.parametrize("prec", PREC, ids=PREC_IDS)
def test_relative_chol6_and_solve6(prec, bounds):
    """L by its backward residual, lndet, y and d^2 within their bounds; ok is the verdict; the identity part is exact"""
    maxima, fails = _chol(prec)
    _report("chol6", maxima)
    assert not _split(fails, bounds), _split(fails, bounds)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PREC, ids=PREC_IDS)
def test_d0sq_is_robust_eval_at_one(prec):
    """same bits, on every record of every table of robust_scale"""
    for case in ("contracts", "benign_loose", "spread", "gated"):
        tb, _ = sr.scale_case(prec, case)
        X = tb.X.copy()
        X[:, sr.SR_LAM] = 1.0
        f = device("eval", prec, X)[:, 0]
        d0 = run("scale", prec, case)[:, 2]
        assert np.array_equal(np.isnan(f), np.isnan(d0)) and np.array_equal(f[~np.isnan(f)].view(np.int64), d0[~np.isnan(d0)].view(np.int64)), case


def _nan_record():
    r = np.full(sr.IN, np.nan)
    r[sr.SR_M], r[sr.SR_ELIGIBLE] = 3.0, 1.0        # (the device converts m to an integer)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("prim", ["eval", "scale", "chol6", "solve"])
@pytest.mark.parametrize("prec", PREC, ids=PREC_IDS)
def test_neighbour_independence(prec, prim):
    """bit-exact: a lane's result does not depend on the regime, the trip count or the NaN of the other lanes of its wavefront"""
    tb, rl = _table(prim, prec, "mixed")
    assert len(set(tb.cls.tolist())) >= 2
    src, base = placements(tb.cls)
    Y = device(prim, prec, np.where(src[:, None] >= 0, tb.X[np.maximum(src, 0)], _nan_record()[None, :]), rl)
    bits = lambda A: np.ascontiguousarray(A).view(np.int64)
    Yb = Y[base]
    moved = np.nonzero((src >= 0) & np.any(bits(Y) != bits(Yb)[np.maximum(src, 0)], axis=1))[0]
    assert moved.size == 0, (moved.size, [(tb.names[tb.reg[src[i]]], int(i % 64), Y[i, :7].tolist(), Yb[src[i], :7].tolist()) for i in moved[:4]])
    n = len(tb.X) - (1 if len(tb.X) % 64 == 0 else 0)          # table order, the last wavefront ragged
    Yr = device(prim, prec, tb.X[:n], rl)
    ragged = np.nonzero(np.any(bits(Yr) != bits(Yb[:n]), axis=1))[0]
    assert ragged.size == 0, (ragged[:4].tolist(), Yr[ragged[:4], :7].tolist(), Yb[ragged[:4], :7].tolist())
    if prim == "scale":      # the launch mixes trip counts: the step counts of the table differ
        assert len(set(Yb[:, 1].tolist())) >= 4
