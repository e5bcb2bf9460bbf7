"""The plain NumPy statements the parity tests of the bearing, sensor-frame, association and sampled features rely on --
bearing_reference.s2_log, s2_exp and direction, sensor_meas_reference.h, a float64 / float32 forward substitution and a NumPy
cos_sinc_sqrt -- against the 40-digit references of tests/meas_primitives_reference.py, on the case tables the device is run on
(tests/test_gpu_meas_primitives.py).  No GPU.

Their largest errors per primitive, precision and regime, in the units of the helper's docstring, are the first column of
profiles/meas_primitives_parity.txt (reference-alone / bound / device); the device's bounds derive from them and from nothing
the device returned.  Here they are held to what is written there (two digits, rounded up with 5 % to spare).  As measured:

    s2_log     0.70 over theta = 1e-12 ... pi - 1e-8 (4.3 with |u| or |v| 4 ulp off 1: the double projection is tangent to the
               u it is given, the reference is the header's literal v - (u.v) u)
    s2_exp     3.5 up to |w| = 10
    direction  2.3 (POSE_POINT, ranges 1e-3 ... 1e7 m and the cancelling lever arm)
    sensor h   5.0 (POSE_POINT, ORIENT_SPECIFIC_FORCE)
    solves     0.76 of (|Ls^-1| |Ls| |y|)_k

The contracts of the sphere logarithm -- tangent over the whole range, length theta, exact zeros at v = u, NaN in NaN out, a tangent
vector of length pi at the antipode -- are asserted on the NumPy statement as they are on the device.  bearing_reference.s2_log as
it stood before it projected twice fails the tangency assertion on 168 of the 421 records (47 of `small`, radial share up to
1e12 eps at theta = 1e-12; 3 of `mid` at theta = 0.1; 83 of `near_pi`, every k, 1e8 eps at pi - 1e-8; 3 of `antipode`, all of w
at v = -u for a generic u; 32 of `offunit`), the length at v = -u (it returned pi u, or zeros), and
NaN in, NaN out (it returned zeros)."""
import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import meas_primitives_reference as mr  # noqa: E402
from probe_support import DT, EPS, F32, F64  # noqa: E402

IDS = [mr.case_id(c) for c in mr.CASES]


@pytest.fixture(scope="module")
def listed():
    return mr.profile_table()


@pytest.mark.parametrize("case", mr.CASES, ids=IDS)
def test_numpy_statement_against_40_digits(case, listed):
    """the reference-alone maxima: at most what profiles/meas_primitives_parity.txt lists, from which the device's bounds derive"""
    e = mr.errors(case, mr.numpy_statement(case))
    row = listed[mr.case_id(case)]
    seen = mr.by_regime(case, e)
    assert set(seen) == set(row), "every regime has inputs and a line"
    for r, v in seen.items():
        print(f"MEAS reference-alone {mr.case_id(case)} {r}: {v:.3g}")
        assert v <= row[r][0], (r, v, row[r])


def test_table_follows_its_rule(listed):
    """a bound's first term is four times the reference-alone maximum with a floor of 4 units, whatever the device showed"""
    assert set(listed) == set(IDS)
    for cid, row in listed.items():
        for r, (ref, bound, dev) in row.items():
            assert bound == mr.base_bound(ref), (cid, r)


def test_numpy_s2_log_contracts(listed):
    case = mr.CASES[0]
    tb = mr.table(case)
    Y = mr.numpy_statement(case)
    name = lambda n: tb.reg == tb.names.index(n)
    radial, length = mr.log_contract_values(Y)
    fin = ~name("nan")
    bad = np.nonzero(fin & ~(radial <= 8.0))[0]
    assert bad.size == 0, [(tb.names[tb.reg[i]], int(i), float(radial[i])) for i in bad[:8]]
    bad = np.nonzero(fin & ~(length <= mr.record_bounds(case, listed) * mr.reference(case)[2][:, 0]))[0]
    assert bad.size == 0, [(tb.names[tb.reg[i]], int(i), float(length[i])) for i in bad[:8]]
    assert np.all(Y[name("same"), :3] == 0.0)
    assert np.isnan(Y[name("nan"), :3]).all()
    anti = name("antipode")
    assert anti.sum() >= 18 and np.isfinite(Y[anti, :3]).all()


def test_numpy_s2_exp_contracts(listed):
    case = mr.CASES[1]
    Y = mr.numpy_statement(case)[:, :3].astype(np.longdouble)
    assert np.abs(np.sqrt(np.sum(Y * Y, axis=1)) - 1).max() <= 2 * EPS[F64]
    import bearing_reference as br
    tb = mr.table(mr.CASES[0])
    fin = np.isfinite(tb.X[:, :6]).all(axis=1)
    u, v = tb.X[fin, 0:3], tb.X[fin, 3:6]
    back = br.s2_exp(u, br.s2_log(u, v))
    assert np.all(np.abs(back - v).max(axis=1) <= EPS[F64] * mr.roundtrip_bounds(listed)[fin])


def test_numpy_flags_and_entries_beyond_m():
    for orient in (False, True):
        case = ("bearing_orient" if orient else "bearing_pose", F64, 0)
        tb = mr.table(case)
        flag = tb.reg == tb.names.index("flag")
        assert flag.sum() >= 4 and np.array_equal(mr.numpy_statement(case)[:, 3], np.where(flag, 0.0, 1.0))
    for case in mr.CASES:
        if case[0] == "solve6":
            tb, m = mr.table(case), case[2]
            Y = mr.numpy_statement(case)
            assert np.array_equal(Y[:, m:], np.broadcast_to(mr.SENTINEL + np.arange(m, 6), Y[:, m:].shape))
            assert np.isfinite(Y[:, :m]).all() and (m == 6 or (np.isnan(tb.X[:, 27 + m:33]).all() and np.isnan(tb.X[:, 6 + m * (m + 1) // 2:27]).all()))


def test_tables_sit_where_the_issue_puts_them():
    """records exact in T; the edges to the bit; every regime and class present"""
    lg = mr.log_table()
    u, v = lg.X[:, 0:3], lg.X[:, 3:6]
    assert len(lg.X) % 64 != 0   # (the ragged launch of the device test ends inside a wavefront)
    for x in mr._ulps(0.6, 3, np.float64):
        assert (np.abs(u[:, 0]) == float(x)).any()
    for e in np.eye(3):
        assert (u == e).all(axis=1).any() and (u == -e).all(axis=1).any()
    assert ((u == [1.0, 0.0, 0.0]).all(axis=1) & (v == [1.0, 1e-170, 0.0]).all(axis=1)).any()
    anti = lg.reg == lg.names.index("antipode")
    assert np.array_equal(v[anti], -u[anti]) and (np.abs(u[anti]).max(axis=1) < 1).sum() >= 4
    th = mr.reference(mr.CASES[0])[4]
    near = lg.reg == lg.names.index("near_pi")
    for k in range(1, 9):
        assert (np.abs((np.pi - th[near]) / 10.0 ** -k - 1) < 1e-6).any(), k
    for t in mr.LOG_SMALL:
        assert (np.abs(th[lg.reg == lg.names.index("small")] / t - 1) < 1e-3).any(), t
    n2 = np.sum(lg.X[lg.reg == lg.names.index("offunit"), 0:6].reshape(-1, 2, 3).astype(np.longdouble) ** 2, axis=2)
    off = 0.5 * np.abs(n2 - 1).max(axis=1) / 2.0 ** -53           # | |x| - 1 | of the vector that was moved, in ulp of 1-
    assert (off > 2.5).all() and (off < 6).all(), off
    for prec in (F64, F32):
        T = DT[prec]
        x2 = mr.cos_sinc_table(prec).X[:, 0]
        assert np.array_equal(x2.astype(T).astype(np.float64), x2)
        for x in mr._ulps(mr.TAYLOR[prec], 3, T) + [0.0, 100.0]:
            assert float(x) in x2
        for m in range(1, 7):
            X = mr.solve_table("solve6", prec, m).X
            fin = np.isfinite(X)
            assert np.array_equal(np.where(fin, X, 0).astype(T).astype(np.float64), np.where(fin, X, 0))
    w = np.linalg.norm(mr.exp_table().X[:, 3:6], axis=1)
    for n in (0.0, 1e-160, 1e-12, 1e-8, 1e-4, 0.1, 3.0, 4.0, 6.0, 10.0):
        assert (np.abs(w - n) <= 1e-3 * n).any(), n   # (the squares of 1e-160 are subnormal)
    for orient in (False, True):
        sb = mr.sensor_table(orient)
        assert sorted(set(sb.raw.ids.tolist())) == ([5, 6, 7] if orient else [0, 1, 2, 3, 4])
        bt = mr.bearing_table(orient)
        assert set(bt.reg.tolist()) == set(range(len(bt.names))) - ({bt.names.index("cancel")} if orient else set())
    bt = mr.bearing_table(False)
    unit = mr.reference(("bearing_pose", F64, 0))[2][:, 0]
    assert np.all(np.abs(unit[bt.reg == bt.names.index("cancel")] / 1e6 - 1) < 0.05)   # |d| = 1e-6 (|b - p| + |r|)
