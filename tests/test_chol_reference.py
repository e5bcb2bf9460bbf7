"""The reference side of tests/test_gpu_chol_primitive.py on the CPU: the bound B and the margin m of tests/chol_reference.py
are legitimate before any device run.

 * a NumPy emulation in T of the recurrence chol16 publishes (trailing update by a rcp(pivot), unscaled columns, rs =
   rsqrt(pivot) at the end), its reciprocal and reciprocal square root perturbed by random relative errors up to the pinned
   primitive bounds, stays inside B on every finite family.  This checks the bound; it measures nothing about the kernel.
 * every clearly-PD input has lambda_min(H) >= m, every clearly-indefinite one lambda_min(H) <= -m, none lies between: the
   share of inputs excluded from a verdict is zero by construction.
 * the emulation's verdict is right on all of them, for the short factorisations (KS < D) too."""
import numpy as np
import pytest

pytest.importorskip("mpmath")

import chol_reference as R  # noqa: E402

CASES = [(p, d) for p in (R.F64, R.F32) for d in (12, 13)]
IDS = [f"{'f64' if p == R.F64 else 'f32'}-D{d}" for p, d in CASES]
SHORT = {12: (6,), 13: (6, 3)}      # KS of the short variants (tests/cpp/chol_probe.hip VARIANTS)


def test_bound_values():
    """the numbers the docstrings quote, and monotonicity in j"""
    assert abs(R.B(R.F64, 13, 12) / R.EPS[R.F64] - 78.5) < 0.01 and abs(R.B(R.F32, 13, 12) / R.EPS[R.F32] - 12.5) < 0.01
    for prec, D in CASES:
        b = [R.B(prec, D, j) for j in range(D)]
        assert all(x < y for x, y in zip(b, b[1:]))
        # never looser than Thm 10.3's gamma_{D+1} with u replaced by the per-term error (one rcp, two rsqrt, D + 1 roundings)
        ueff = R.U[prec] + 3 * R.PRIM_EPS[prec] * R.EPS[prec] / (D + 1)
        assert b[-1] <= (D + 1) * ueff / (1 - (D + 1) * ueff) * 1.001
        assert R.margin(prec, D) == D * b[-1]
    assert R.cond_decades(R.F64, 13)[-1] == 12 and R.cond_decades(R.F32, 13)[-1] == 4


@pytest.mark.parametrize("prec,D", CASES, ids=IDS)
def test_reference_factor(prec, D):
    """ref_chol reproduces its input to the reference precision and agrees with LAPACK where that is accurate"""
    A = R.family("well", prec, D)[:12]
    for a in A:
        L = R.ref_chol(a, prec)
        assert np.abs(R.residual(a, L, prec)).max() <= 4 * D * 2.0 ** -53 * np.abs(a).max()
        assert np.abs(L - np.linalg.cholesky(a)).max() <= 1e-13 * np.abs(L).max()
    assert R.ref_chol(R.family("indef", prec, D)[0], prec) is None


@pytest.mark.parametrize("prec,D", CASES, ids=IDS)
def test_no_input_in_the_band(prec, D):
    for name in R.FINITE_PD:
        c = R.classes(name, prec, D)
        assert len(c) >= 100 and (c == 1).all(), (name, np.nonzero(c != 1)[0][:8].tolist())
    c = R.classes("indef", prec, D)
    assert (c == -1).all(), np.nonzero(c != -1)[0][:8].tolist()
    # a first failing pivot at p leaves every leading block up to p clearly PD: what the short variants are asked about
    pos = R.indef_position(D)
    assert sorted(set(pos.tolist())) == list(range(D))
    for KS in SHORT[D]:
        c = R.classes("indef", prec, D, KS)
        assert (c[pos >= KS] == 1).all() and (c[pos < KS] == -1).all(), KS
    excluded = sum(int((R.classes(n, prec, D) == 0).sum()) for n in R.FINITE_PD + ("indef",))
    assert excluded == 0


@pytest.mark.parametrize("prec,D", CASES, ids=IDS)
def test_emulated_recurrence_stays_inside_the_bound(prec, D):
    rng = np.random.default_rng(7 + prec + D)
    Bm = R.B_matrix(prec, D)
    worst = {}
    for name in R.FINITE_PD:
        A = R.family(name, prec, D)
        v, rs, ok = R.emulate(A, prec, rng)
        assert ok.all(), name
        # fp64: the 40-digit residual of every sixth record (the emulation is a check on the bound; the device test takes all)
        step = 6 if prec == R.F64 else 1
        w = 0.0
        for a, vi, ri in zip(A[::step], v[::step], rs[::step]):
            res = np.abs(R.residual_from_device(a, vi, ri, prec))
            d = np.sqrt(np.diag(a))
            w = max(w, float((res / (Bm * np.outer(d, d))).max()))
        worst[name] = w
        assert w <= 1.0, worst
    print("emulation: worst |A - L L^T| / bound per family", worst)


@pytest.mark.parametrize("prec,D", CASES, ids=IDS)
def test_emulated_verdict(prec, D):
    rng = np.random.default_rng(11 + prec + D)
    pos = R.indef_position(D)
    for KS in (D,) + SHORT[D]:
        for name in R.FINITE_PD:
            assert R.emulate(R.family(name, prec, D), prec, rng, KS)[2].all(), (name, KS)
        ok = R.emulate(R.family("indef", prec, D), prec, rng, KS)[2]
        assert (ok == (pos >= KS)).all(), (KS, np.nonzero(ok != (pos >= KS))[0][:8].tolist())
    for name in ("zero_row",):
        A, p = R.special(name, prec, D)
        assert not R.emulate(A, prec, rng)[2].any()
