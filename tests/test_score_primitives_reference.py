"""The references, tables and NumPy statements of tests/score_primitives_reference.py, on the CPU: known answers, the verdict
margins, the conditions under which a step count is determined, the table of profiles/score_primitives_parity.txt against a fresh
measurement, and every assertion of tests/test_gpu_score_primitives.py applied to the NumPy statements in T of the same primitives
on the same tables.  No GPU.

As measured, the NumPy statement of the pivot chain stays below 2.6 units of f (kappa_H f_ref) and 4.1 of g over kappa_H = 1 ...
1e13 (fp64) and 1 ... 1e5 (fp32): the unit flattens the decades.  Its MATCH residual stays within 0.1 slack of the root on every
record, generalised-eigenvalue spreads of 1e8 included, and it never reaches the step cap of 64."""
import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import score_primitives_reference as sr  # noqa: E402
from probe_support import DT, EPS, F32, F64  # noqa: E402

PREC = [F64, F32]
PREC_IDS = ["f64", "f32"]


@pytest.fixture(scope="module")
def listed():
    return sr.profile_table()


@pytest.fixture(scope="module")
def maxima():
    return sr.numpy_maxima()


def test_numpy_statements_against_40_digits(maxima, listed):
    """the reference-alone maxima: at most what the profile lists, from which the device's bounds derive"""
    assert set(listed) == set(sr.LINE_IDS) == set(maxima)
    for lid in sr.LINE_IDS:
        assert set(maxima[lid]) == set(listed[lid]), lid
        for r, v in maxima[lid].items():
            print(f"SCORE reference-alone {lid} {r}: {v:.3g}")
            assert v <= listed[lid][r][0], (lid, r, v, listed[lid][r])
            assert listed[lid][r][0] <= max(1.5 * v, 0.1) or listed[lid][r][0] == 0, ("the listed maximum is stale", lid, r, v, listed[lid][r])


def test_table_follows_its_rule(listed):
    """a bound's first term is four times the reference-alone maximum with a floor of 4 units, whatever the device showed"""
    for lid, row in listed.items():
        for r, (ref, bound, dev) in row.items():
            assert bound == sr.base_bound(ref), (lid, r)


def test_margins_quoted():
    assert abs(sr.margin6(F64) / EPS[F64] / 3.1e2 - 1) < 0.02 and abs(sr.margin6(F32) / EPS[F32] / 45 - 1) < 0.02
    assert sr.cond_decades(F64, sr.margin6(F64))[-1] == 12 and sr.cond_decades(F32, sr.margin6(F32))[-1] == 4
    assert sr.cond_decades(F64, sr.margin3(F64))[-1] == 13 and sr.cond_decades(F32, sr.margin3(F32))[-1] == 5
    for prec in PREC:
        assert all(sr.B6(prec, j) < sr.B6(prec, j + 1) for j in range(5))
        assert sr.margin3(prec) > 3 * (3 * 0.5 + sr.RECIP[prec]) * EPS[prec]        # three roundings and the reciprocal, per entry


@pytest.mark.parametrize("prec", PREC, ids=PREC_IDS)
def test_every_record_has_a_verdict(prec):
    """clearly positive definite or clearly indefinite by the margins of the helper's docstring: nothing in between"""
    T = DT[prec]
    tb, ref = sr.eval_table(prec), sr.eval_reference(prec)
    fin = np.isfinite(tb.X).all(axis=1)
    assert np.array_equal(tb.X[fin, :16].astype(T).astype(np.float64), tb.X[fin, :16])
    ind = tb.reg == tb.names.index("indefinite")
    assert (ref["pd"][ind] == -1).all() and (ref["pd"][fin & ~ind] == 1).all() and ind.sum() >= 12 and (~fin).sum() == 16
    k = ref["kappa"]
    assert k[tb.reg == tb.names.index("random")].max() <= 10.0
    ill = np.log10(k[tb.reg == tb.names.index("illcond")])
    assert set(sr.cond_decades(prec, sr.margin3(prec))) <= set(np.round(ill).astype(int).tolist()) | {1}      # (scaling may lower a draw's decade)
    for name in sr.SCALE_TABLES:
        tbs, first = sr.scale_table(prec, name), sr.scale_first(prec, name)
        fin = np.isfinite(tbs.X).all(axis=1)
        ind = np.zeros(len(tbs.X), bool) if "s1_indefinite" not in tbs.names else tbs.reg == tbs.names.index("s1_indefinite")
        assert (first["pd"][ind] == -1).all() and (first["pd"][fin & ~ind] == 1).all(), name
    assert np.nanmax(sr.scale_first(prec, "benign")["kappa1"]) <= (1e3 if prec == F64 else 10.0)
    tb, ref = sr.chol_table(prec), sr.chol_reference(prec)
    pdm = sr.pd_mask(tb, sr.PD6)
    ind = tb.reg == tb.names.index("indefinite")
    assert (ref["pd"][pdm] == 1).all() and (ref["pd"][ind] == -1).all() and ind.sum() == 36
    fin = np.isfinite(tb.X).all(axis=1)
    assert np.array_equal(tb.X[fin].astype(T).astype(np.float64), tb.X[fin])
    ill = np.log10(ref["kappa"][tb.reg == tb.names.index("illcond")])
    assert set(sr.cond_decades(prec, sr.margin6(prec))) <= set(np.round(ill).astype(int).tolist()) | {1}
    for i in np.nonzero(tb.reg == tb.names.index("semidefinite"))[0]:      # a zero row and column, the rest clearly positive definite
        A = sr.unpack(tb.X[i, :21], 6)
        p = np.nonzero(np.diag(A) == 0)[0]
        assert p.size == 1 and not A[p[0]].any() and not A[:, p[0]].any()
        keep = [j for j in range(6) if j != p[0]]
        assert sr.classify(A[np.ix_(keep, keep)].tolist(), sr.margin6(prec)) == 1
    assert len(tb.X) % 64 != 0 and len(sr.eval_table(prec).X) % 64 != 0      # (the ragged launch ends inside a wavefront)


@pytest.mark.parametrize("prec", PREC, ids=PREC_IDS)
def test_known_answers(prec):
    tb, ref = sr.eval_table(prec), sr.eval_reference(prec)
    for i in np.nonzero(tb.reg == tb.names.index("identity"))[0]:
        r = tb.X[i]
        assert abs(ref["f"][i, 0] / (np.dot(r[12:15], r[12:15]) / (1 + r[sr.SR_LAM] * r[6])) - 1) < 1e-15
    for i in np.nonzero(tb.reg == tb.names.index("m1"))[0]:
        r = tb.X[i]
        s = r[0] + r[sr.SR_LAM] * r[6]
        assert abs(ref["f"][i, 0] / (r[12] ** 2 / s) - 1) < 1e-15 and abs(ref["g"][i, 0] / (r[12] ** 2 * r[6] / s ** 2) - 1) < 1e-15
    tb, rl = sr.scale_case(prec, "contracts")
    nr = sr.newton_reference(prec, "contracts")
    c1 = rl.chi2_m1
    for i in np.nonzero(tb.reg == tb.names.index("m1"))[0]:          # lambda* = (nu^2 / c^2 - s) / q, reached in one exact step
        r = tb.X[i]
        assert nr["its"][i] == 1 and abs(nr["root"][i] / ((r[12] ** 2 / c1 - r[0]) / r[6]) - 1) < 1e-13 and abs(nr["resid"][i][1]) < 1e-30
    first = sr.scale_first(prec, "contracts")
    for i in np.nonzero(tb.reg == tb.names.index("proportional"))[0]:    # Q = t Sigma_z up to its rounding: ((1 + t) f(1) / c^2 - 1) / t
        t = tb.X[i, 6] / tb.X[i, 0]
        assert nr["its"][i] == 1 and abs(nr["root"][i] / (((1 + t) * first["f1"][i, 0] / rl.chi2_m3 - 1) / t) - 1) < 64 * EPS[prec]
    with mp.workdps(40):
        for i in np.nonzero(tb.reg == tb.names.index("null"))[0]:       # S(1)^-1 nu in the null space of Q: g = 0 exactly
            f, g, _ = sr.mp_eval(tb.X[i], 1.0)
            assert g == 0 and f > rl.chi2_m3
    tbc, refc = sr.chol_table(prec), sr.chol_reference(prec)
    idn = tbc.reg == tbc.names.index("identity")
    assert (refc["lndet"][idn, 0] == 0).all() and np.array_equal(refc["y"][idn, :, 0], tbc.X[idn, 21:27])
    i = int(np.nonzero(tbc.reg == tbc.names.index("random"))[0][0])
    A, v = sr.unpack(tbc.X[i, :21], 6), tbc.X[i, 21:27]
    assert abs(refc["lndet"][i, 0] / np.linalg.slogdet(A)[1] - 1) < 1e-12 and abs(refc["d2"][i, 0] / (v @ np.linalg.solve(A, v)) - 1) < 1e-10


@pytest.mark.parametrize("prec", PREC, ids=PREC_IDS)
def test_step_counts_are_determined_where_asserted(prec, listed):
    """on the reference alone: the root within max_iter / 2 steps on benign and spread; m1, proportional and benign at the loose
    tolerance unambiguous on every record; inliers and gated rows clear of their thresholds; the clamp's roots above scale_max"""
    for case in ("benign_loose", "benign_tight", "spread"):
        tb, rl = sr.scale_case(prec, case)
        nr = sr.newton_reference(prec, case)
        assert tb.match.all() and nr["reached"].all() and nr["pd"].all() and nr["its"].max() <= rl.max_iter // 2, (case, nr["its"].max())
    for case, names in (("contracts", ("m1", "proportional")), ("benign_loose", ("q1", "q1e-6"))):
        tb, rl = sr.scale_case(prec, case)
        un = sr.unambiguous(prec, case, sr.scale_fbound(prec, case, listed))
        rows = sr.pd_mask(tb, names)
        assert rows.sum() >= 54 and un[rows].all(), (case, int((~un[rows]).sum()))
    tb, rl = sr.scale_case(prec, "contracts")
    first, fb = sr.scale_first(prec, "contracts"), sr.scale_fbound(prec, "contracts", listed)
    inl = tb.reg == tb.names.index("inlier")
    c2 = np.where(tb.X[:, sr.SR_M] == 1, rl.chi2_m1, rl.chi2_m3)
    assert (first["f1"][inl, 0] < c2[inl] * (1 - 2 * fb[inl] * EPS[prec] * first["kappa1"][inl])).all()
    out = tb.match | sr.pd_mask(tb, ("null", "ineligible", "indefinite_q"))
    assert (first["f1"][out, 0] > c2[out] * (1 + 2 * fb[out] * EPS[prec] * first["kappa1"][out])).all()
    tb, rl = sr.scale_case(prec, "gated")
    first, fb = sr.scale_first(prec, "gated"), sr.scale_fbound(prec, "gated", listed)
    gated = tb.reg == tb.names.index("gated")
    slack = 2 * fb * EPS[prec] * first["kappa1"]
    assert (first["f1"][gated, 0] * (1 - slack[gated]) > rl.gate_chi2).all() and (first["f1"][~gated, 0] * (1 + slack[~gated]) < rl.gate_chi2).all()
    tb, rl = sr.scale_case(prec, "clamp")
    nr = sr.newton_reference(prec, "clamp")
    cl = tb.reg == tb.names.index("clamp")
    assert nr["clamped"][cl].all() and not nr["clamped"][~cl].any() and nr["reached"][~cl].all() and (nr["root"][~cl] < rl.scale_max / 1.5).all()
    with mp.workdps(40):
        assert all(sr.mp_eval(tb.X[i], 1.5 * rl.scale_max)[0] > rl.chi2_m3 for i in np.nonzero(cl)[0])
    tb, rl = sr.scale_case(prec, "mixed")
    assert len(set(sr.newton_reference(prec, "mixed")["its"].tolist())) >= 5          # the launch mixes trip counts


@pytest.mark.parametrize("prec", PREC, ids=PREC_IDS)
def test_numpy_statements_hold_the_device_assertions(prec, listed):
    """every bound and contract of tests/test_gpu_score_primitives.py, on the NumPy statements in T"""
    T = DT[prec]
    _, fails = sr.eval_failures(prec, sr.np_eval_outputs(prec), listed)
    assert not fails, fails
    tb = sr.chol_table(prec)
    _, fails = sr.chol_failures(prec, sr.np_chol6(tb.X, T), sr.np_chol6(tb.X, T, solve=True), listed)
    assert not fails, fails
    for case in sr.SCALE_CASES:
        tbs, rl = sr.scale_case(prec, case)
        _, lines, fails = sr.scale_failures(prec, case, sr.np_scale(tbs.X, rl, T), listed)
        assert not fails, (case, fails)


def test_assertions_notice_a_wrong_answer(listed):
    """the assertions are not vacuous: a lambda one part in 1e6 past the root, a step too many, a flipped verdict, a padded entry
    off by one ulp and a pivot chain that loses half its digits each fail"""
    tb, rl = sr.scale_case(F64, "benign_tight")
    Y = sr.np_scale(tb.X, rl, np.float64)
    Z = Y.copy()
    Z[:, 0] *= 1 + 1e-6
    assert any(f[0] == "-slack <= r <= tol + slack" for f in sr.scale_failures(F64, "benign_tight", Z, listed)[2])
    tb, rl = sr.scale_case(F64, "benign_loose")
    Z = sr.np_scale(tb.X, rl, np.float64)
    Z[0, 1] += 1
    assert any(f[0] == "its == its_ref" for f in sr.scale_failures(F64, "benign_loose", Z, listed)[2])
    Z = sr.np_eval_outputs(F64)
    Z[:, 0] *= 1 + 1e-8
    assert any(f[0] == "f" for f in sr.eval_failures(F64, Z, listed)[1])
    tbc = sr.chol_table(F64)
    Y, Ys = sr.np_chol6(tbc.X, np.float64), sr.np_chol6(tbc.X, np.float64, solve=True)
    Z = Y.copy()
    Z[:, 27] = 1.0
    assert any(f[0] == "chol6: ok is the verdict" for f in sr.chol_failures(F64, Z, Ys, listed)[1])
    Z = Y.copy()
    i = int(np.nonzero(tbc.reg == tbc.names.index("padded"))[0][0])
    Z[i, 20] = np.nextafter(1.0, 2.0)
    assert any(f[0] == "padded entries are exact" for f in sr.chol_failures(F64, Z, Ys, listed)[1])
    Z = Y.copy()
    Z[:, 28] += 1e-9
    assert any(f[0] == "lndet" for f in sr.chol_failures(F64, Z, Ys, listed)[1])


def test_numpy_statements_agree_with_the_robust_reference():
    """np_eval and np_scale in float64 against tests/robust_reference.py (evaluate: LAPACK solves; newton_iterates: the kernel's rule
    restated) on the benign regime"""
    import robust_reference as rr
    tb, rl = sr.scale_case(F64, "benign_loose")
    Sz, Q, nu = sr.unpack(tb.X[:, 0:6], 3), sr.unpack(tb.X[:, 6:12], 3), tb.X[:, 12:15]
    kap = sr.scale_first(F64, "benign")["kappa1"]
    for lam in (1.0, 7.0, 1e5):
        f, g, ok = sr.np_eval(tb.X, np.full(len(tb.X), lam), np.float64)
        f2, g2 = rr.evaluate(Sz, Q, nu, np.full(len(tb.X), lam))
        assert ok.all() and (np.abs(f / f2 - 1) <= 1e-12 * kap).all() and (np.abs(g / g2 - 1) <= 1e-12 * kap).all()
    Y = sr.np_scale(tb.X, rl, np.float64)
    it, steps = rr.newton_iterates(Sz, Q, nu, rl.chi2_m3, rl.tol, rl.max_iter, rl.scale_max)
    assert np.array_equal(Y[:, 1], steps) and (np.abs(Y[:, 0] / it[:, -1] - 1) <= 1e-10).all()
