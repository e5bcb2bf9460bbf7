"""tests/scaled_parity.py pinned on the CPU: known answers for the metric and the bounds, the measurement of M (the spread between
two independent correct fp32 evaluations: the C++ float oracle and the all-float32 NumPy evaluation of tests/study_f32_mixed.py),
the statuses of both oracles on the input sets of tests/test_gpu_scaled_parity.py, and five subtly wrong results that the old
max |x - ref| <= 1e-4 passes and the scaled check refuses."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scaled_parity as sp  # noqa: E402
from conftest import max_abs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ the metric
def test_metric_hand_built_two_filters(spe, oracle):
    s = np.array([0.1] * 3 + [0.05] * 3 + [0.2] * 3 + [0.02] * 3)
    mu_o, _ = spe.synth.pose_initial(2)
    C_o = np.stack([np.diag(s * s), np.diag(4.0 * s * s)])          # filter 1: twice the sigmas
    delta = np.zeros((2, 12))
    delta[0, 1], delta[0, 4], delta[0, 11] = 0.01, -0.001, 0.004    # 0.1, 0.02, 0.2 sigma
    delta[1, 1], delta[1, 7] = 0.03, 0.1                            # 0.15, 0.25 sigma (sigmas doubled)
    mu = np.stack([oracle.pose_boxplus(mu_o[k], delta[k]) for k in range(2)])
    C = C_o.copy()
    C[0, 0, 9] = C[0, 9, 0] = 1e-4                                  # / (0.1 * 0.02) = 0.05
    C[1, 6, 6] += 0.08                                              # / 0.4^2 = 0.5
    C[1, 3, 7] = C[1, 7, 3] = -0.01                                 # / (0.1 * 0.4) = 0.25
    d = sp.distances("pose", mu, C, mu_o, C_o)
    assert np.allclose(d.mean, [0.15, 0.02, 0.25, 0.2], rtol=1e-9, atol=1e-12) and list(d.mean_at) == [1, 0, 1, 0]
    want = np.zeros((4, 4))
    want[0, 3] = want[3, 0] = 0.05
    want[2, 2] = 0.5
    want[1, 2] = want[2, 1] = 0.25
    assert np.allclose(d.cov, want, rtol=1e-12, atol=1e-15)
    assert d.cov_at[0, 3] == 0 and d.cov_at[2, 2] == 1 and d.cov_at[1, 2] == 1
    assert len(d.items()) == 4 + 10
    # the filter index is the batch's when rows are a subset
    d2 = sp.distances("pose", mu, C, mu_o, C_o, filters=[40, 77])
    assert list(d2.mean_at) == [77, 40, 77, 40]
    # the bound names block, filter, value and bound
    b = sp.Bound(np.full(4, 0.3), np.full((4, 4), 0.3))
    assert sp.violations(d, b) == [("cov[velocity,velocity]", 1, pytest.approx(0.5), 0.3)]
    with pytest.raises(AssertionError, match=r"block cov\[velocity,velocity\] filter 1: 5.000e-01 > bound 3.000e-01"):
        sp.check(d, b, "x")
    nan = sp.Dist("pose", d.mean * np.nan, d.cov, d.mean_at, d.cov_at)
    assert len(sp.violations(nan, sp.Bound(np.full(4, 1.0), np.full((4, 4), 1.0)))) == 4


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_metric_identity_and_scaled_block(spe, model):
    c = sp.Case(spe, model, "f64", 7)
    d = sp.distances(model, c.mu, c.cov, c.mu, c.cov)
    assert (d.mean == 0).all() and (d.cov == 0).all()
    assert len(d.items()) == (4 + 10 if model == "pose" else 5 + 15)
    eps = 1e-3
    for k, (name, lo, hi) in enumerate(sp.BLOCKS[model]):
        C = c.cov.copy()
        C[:, lo:hi, lo:hi] *= 1.0 + eps
        s = np.sqrt(np.einsum("nii->ni", c.cov))
        per = np.abs(C - c.cov) / (s[:, :, None] * s[:, None, :])
        assert np.allclose(np.einsum("nii->ni", per)[:, lo:hi], eps, rtol=1e-9)         # every diagonal entry of the block: eps
        d = sp.distances(model, c.mu, C, c.mu, c.cov)
        want = np.zeros_like(d.cov)
        want[k, k] = eps
        assert np.allclose(d.cov, want, rtol=1e-9, atol=0) and (d.mean == 0).all(), name


def test_bounds_known_answers(spe):
    mu_o, _ = spe.synth.orient_initial(2)
    mu_o[0, 4:7] = [0.5, -3.0, 0.2]
    mu_o[1, 4:7] = [0.1, 0.1, -8.0]
    s = np.array([0.05] * 3 + [0.1] * 3 + [0.001] * 3 + [0.01] * 3 + [0.01])
    C_o = np.stack([np.diag(s * s)] * 2)
    v = sp.mean_scale("orient", mu_o, C_o)
    assert np.allclose(v, [2 / 0.05, 8.0 / 0.1, 1 / 0.001, 1 / 0.01, 9.81 / 0.01])
    u = 2.0 ** -24
    w = sp.bound_wide("orient", mu_o, C_o, 3)
    assert np.allclose(w.mean, 6 * u * v + 1e-9) and np.allclose(w.cov, 6 * u + 1e-9)
    assert (sp.bound_f64("orient").mean == 1e-9).all() and (sp.bound_f64("pose").cov == 1e-9).all()
    zero = sp.Dist("orient", np.zeros(5), np.zeros((5, 5)), None, None)
    f = sp.bound_f32("orient", mu_o, C_o, zero)
    assert np.allclose(f.mean, 20 * u * v) and np.allclose(f.cov, 20 * u)
    assert 1.0e-3 < f.mean[4] < 1.3e-3                  # gravity: 9.81 at sigma 0.01 -- fp32 resolves the mean to ~1e-3 sigma
    big = sp.Dist("orient", np.full(5, 1e-2), np.full((5, 5), 1e-3), None, None)
    f = sp.bound_f32("orient", mu_o, C_o, big)
    assert np.allclose(f.mean, sp.M * 1e-2) and np.allclose(f.cov, sp.M * 1e-3)


# ------------------------------------------------------------------------------------------------------ M
@pytest.fixture(scope="module")
def spread(spe, oracle):
    return sp.fp32_spread(spe)


def test_margin_constant_covers_the_measured_spread(spread):
    rows, m = spread
    print("\n" + sp.spread_text(rows, m))
    assert m >= 2.0 and sp.M >= m, (sp.M, m)
    assert sp.M <= 1.25 * m, "M is far above what the CPU measures: re-derive it (tools/scaled_parity_report.py --cpu)"
    recorded = [ln for ln in open(os.path.join(ROOT, "profiles", "scaled_parity.txt")) if ln.startswith("M = ")]
    # (the recorded figure is a ratio of fp32 roundings: another NumPy or BLAS summation order may move it a little)
    assert len(recorded) == 1 and abs(float(recorded[0].split()[2]) - m) <= 0.1 * m and sp.M >= float(recorded[0].split()[2]), (recorded, m)


def test_float_oracle_sits_where_the_issue_found_it(spread):
    """between 2e-8 and 1.8e-4 in every block that moves, the largest values in the OrientationState gravity row and column"""
    rows, _ = spread
    moved = [r for r in rows if r[3] > 0]
    assert len(moved) == len(rows) - 2 and all(r[2] in ("mean[angular_velocity]", "mean[gravity]") and r[1] == "predict"
                                               for r in rows if r[3] == 0)
    cov = [r for r in moved if r[2].startswith("cov")]
    assert all(2e-8 <= r[3] <= 2e-4 for r in cov), [r for r in cov if not 2e-8 <= r[3] <= 2e-4]
    top = max(cov, key=lambda r: r[3])
    assert top[0] == "orient" and "gravity" in top[2]


# ------------------------------------------------------------------------------------------------------ inputs of the GPU file
@pytest.mark.parametrize("noise", ["default", "per_filter"])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_both_oracles_report_no_error_on_the_input_sets(spe, model, noise):
    c = sp.Case(spe, model, "f32", 203, noise)
    dt = 0.01
    zs = [c.z_for(c.full3, k) for k in range(3)]
    chains = {"predict": [("predict", dt)], "three cycles": [], "schedule": [("predict", dt), ("update", c.full3, zs[0], c.Q),
                                                                          ("predict", 2 * dt), ("predict", dt), ("update", c.full3, zs[2], c.Q)]}
    for k in range(3):
        chains["three cycles"] += [("predict", dt), ("update", c.full3, zs[k], c.Q), ("commit",)]
    metas = range(9) if model == "pose" else [spe.MEAS_ORIENT_BODYVEL3]
    for m in metas:
        chains[f"update {m}"] = [("update", m, c.z_for(m), c.Q)]
    if model == "pose":
        mods = [spe.synth.pose_mixed_models(c.n, k) for k in range(3)]
        chains["mixed"] = sum(([("predict", dt), ("update", mods[k], c.z_for(mods[k], k), c.Q)] for k in range(3)), [])
    for name, ops in chains.items():
        for prec, narrow in ((0, False), (1, False), (0, True)):
            _, _, st = c.chain(ops, prec, narrow=narrow)
            assert (st & ~np.uint32(sp.ST_INACTIVE) == 0).all(), (name, prec, narrow, np.unique(st))


def test_chain_on_a_subset_of_rows(spe):
    c = sp.Case(spe, "pose", "f32", 64, "per_filter")
    ops = [("predict", 0.01 + 1e-4 * np.arange(64)), ("update", spe.synth.pose_mixed_models(64, 0), c.z, c.Q), ("commit",)]
    rows = np.array([3, 10, 63])
    m, cv, st = c.chain(ops, narrow=True)
    m2, cv2, st2 = c.chain(ops, narrow=True, rows=rows)
    assert np.array_equal(m[rows], m2) and np.array_equal(cv[rows], cv2) and np.array_equal(st[rows], st2)
    assert c.acc.shape[0] == 64 and c.R.shape[0] == 64 and sp.commits(ops) == 1


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_judge_on_cpu_stand_ins(spe, model):
    """the whole check with CPU results in the engine's place: the float oracle as the fp32 engine, the narrowed fp64 chain as the
    wide engine, the fp64 oracle as the fp64 engine; a gyro-bias / angular-velocity block 1e-3 off is named with its filter"""
    dt = 0.01
    for mode, prec in (("f64", 0), ("f32", 1), ("wide", 0)):
        c = sp.Case(spe, model, mode)
        ops = []
        for k in range(3):
            ops += [("predict", dt), ("update", c.full3, c.z_for(c.full3, k), c.Q), ("commit",)]
        assert sp.commits(ops) == 3
        m, cv, st = c.chain(ops, prec, narrow=(mode == "wide"))
        rep = []
        sp.judge(c, ops, m, cv, st, "stand-in", report=rep)
        assert len(rep) == 1 and len(sp.table(rep[0][1], rep[0][2]).splitlines()) == (14 if model == "pose" else 20)
        lo = 9 if model == "pose" else 6
        name = "angular_velocity" if model == "pose" else "gyro_bias"
        cv = cv.copy()
        cv[17, lo, lo] *= 1.0 + 1e-3
        with pytest.raises(AssertionError, match=rf"block cov\[{name},{name}\] filter 17: "):
            sp.judge(c, ops, m, cv, st, "stand-in")
        st = st.copy()
        st[5] = spe.ST_ERR_CHOLESKY
        with pytest.raises(AssertionError, match="status differs from the oracle at filters \\[5\\]"):
            sp.judge(c, ops, m, cv, st, "stand-in")


# ------------------------------------------------------------------------------------------------------ sensitivity
def _old_check(m, c, m_o, c_o):
    return max_abs(m, m_o) <= 1e-4 and max_abs(c, c_o) <= 1e-4


def _blocks_over(model, m, c, ref, d_o32):
    d = sp.distances(model, m, c, *ref)
    return [v[0] for v in sp.violations(d, sp.bound_f32(model, ref[0], ref[1], d_o32))]


@pytest.fixture(scope="module")
def predicted(spe, oracle):
    """one prediction of each bench workload by both oracles"""
    out = {}
    for model in ("pose", "orient"):
        c = sp.Case(spe, model, "f32")
        m64, c64, s64 = c.predict(c.mu, c.cov, 0.01, 0)
        m32, c32, s32 = c.predict(c.mu, c.cov, 0.01, 1)
        assert (s64 == 0).all() and (s32 == 0).all()
        d = sp.distances(model, m32, c32, m64, c64)
        assert _old_check(m32, c32, m64, c64) and not _blocks_over(model, m32, c32, (m64, c64), d)
        out[model] = (c, (m64, c64), (m32, c32), d)
    return out


def test_sensitivity_zeroed_gyro_bias_block(predicted):
    _, ref, (m, c), d = predicted["orient"]
    c = c.copy()
    c[:, 6:9, 6:9] = 0.0
    assert _old_check(m, c, *ref)
    assert _blocks_over("orient", m, c, ref, d) == ["cov[gyro_bias,gyro_bias]"]


def test_sensitivity_gravity_row_scaled(predicted):
    _, ref, (m, c), d = predicted["orient"]
    c = c.copy()
    c[:, 12, :] *= 1.0 + 1e-3
    c[:, :12, 12] = c[:, 12, :12]
    assert _old_check(m, c, *ref)
    # the diagonal entry moves by 1e-3 of itself; the cross blocks by 1e-3 of a correlation, below the float oracle's own 5e-5
    assert _blocks_over("orient", m, c, ref, d) == ["cov[gravity,gravity]"]


def test_sensitivity_swapped_entries_in_the_acc_bias_block(predicted):
    _, ref, (m, c), d = predicted["orient"]
    c = c.copy()
    a, b = c[:, 10, 9].copy(), c[:, 11, 9].copy()
    c[:, 10, 9] = c[:, 9, 10] = b
    c[:, 11, 9] = c[:, 9, 11] = a
    assert _old_check(m, c, *ref)
    assert _blocks_over("orient", m, c, ref, d) == ["cov[acc_bias,acc_bias]"]


def test_sensitivity_dropped_gyro_bias_process_noise(spe, predicted):
    """With orient_process_noise() the gyro-bias noise adds dt^2 1e-10 = 1e-14 to a variance of 1e-6, 1e-8 of it: below what
    fp32 holds (the float oracle's result does not change), so there the fp64 bound has to notice; with the dense noise of
    tests/test_gpu_process_noise.py the fp32 bound does."""
    c, ref, _, _ = predicted["orient"]
    R = c.R.copy()
    R[6:9, 6:9] = 0.0
    m, cv, st = c.predict(c.mu, c.cov, 0.01, 0, R=R)
    assert (st == 0).all() and max_abs(m, ref[0]) <= 1e-9 and max_abs(cv, ref[1]) <= 1e-9         # the old fp64 check
    bad = [v[0] for v in sp.violations(sp.distances("orient", m, cv, *ref), sp.bound_f64("orient"))]
    assert bad == ["cov[gyro_bias,gyro_bias]"]
    Rd = sp.f32r(spe.synth.dense_process_noise("orient"))
    m64, c64, _ = c.predict(c.mu, c.cov, 0.01, 0, R=Rd)
    m32, c32, _ = c.predict(c.mu, c.cov, 0.01, 1, R=Rd)
    d = sp.distances("orient", m32, c32, m64, c64)
    Rd[6:9, 6:9] = 0.0
    m, cv, st = c.predict(c.mu, c.cov, 0.01, 1, R=Rd)
    assert (st == 0).all() and _old_check(m, cv, m64, c64)
    assert _blocks_over("orient", m, cv, (m64, c64), d) == ["cov[gyro_bias,gyro_bias]"]


def test_sensitivity_pose_angular_velocity_block_scaled(predicted):
    _, ref, (m, c), d = predicted["pose"]
    c = c.copy()
    c[:, 9:12, 9:12] *= 1.05
    assert _old_check(m, c, *ref)
    assert _blocks_over("pose", m, c, ref, d) == ["cov[angular_velocity,angular_velocity]"]
