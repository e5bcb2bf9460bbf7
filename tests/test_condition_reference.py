"""Pins for tests/condition_reference.py, the NumPy statement of the covariance conditioning (include/ukf_batch.h) the GPU tests
compare with: healthy input comes back bit for bit; a 2 x 2 indefinite block embedded in the identity has its closed-form answer;
after a repair every eigenvalue of C' is at least eps (1 - 1e-12) and the oracle's Cholesky succeeds; a second application finds
every filter healthy and changes nothing; the eigh form and the literal round-robin Jacobi agree to 1e-12 on C'; the variance
floor behaves as step 2 says; the quaternion renormalisation keeps the direction; the status rules hold one by one; and the
four quarters of the GPU tests are what they claim to be."""
import numpy as np
import pytest

import condition_reference as cr
from engine_support import man_of
from oracle import ukf_numpy as on
from sensor_meas_cases import states

N = 256
EPS = 1e-10


def batch(model, eps=EPS, dtype=np.float64):
    mu, cov, _ = states(model)
    mu, cov = mu[:N], cov[:N]
    bad, v, quarter = cr.make_batch(cov, eps, dtype)
    return man_of(model), mu.astype(dtype).astype(np.float64), bad, v, quarter


def corr_eigs(cov, v):
    C, s, d, raised = cr.correlation(cov, v)
    return np.linalg.eigvalsh(C), raised


@pytest.mark.parametrize("D", [12, 13, 4, 5])
def test_schedule_meets_every_pair_once(D):
    steps = cr.schedule(D)
    DP = (D + 1) // 2 * 2
    assert len(steps) == DP - 1 and all(len(p) == (D // 2 if DP == D else DP // 2 - 1) for p in steps)
    seen = [pq for pairs in steps for pq in pairs]
    assert sorted(seen) == [(p, q) for p in range(D) for q in range(p + 1, D)]
    for pairs in steps:
        flat = [i for pq in pairs for i in pq]
        assert len(set(flat)) == len(flat)   # disjoint


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_healthy_input_comes_back_bit_for_bit(model):
    man = man_of(model)
    mu, cov = states(model)[0][:N], states(model)[1][:N]
    v = 1e-3 * np.einsum("bii->bi", cov).min(axis=0)
    for method in ("eigh", "jacobi"):
        o = cr.condition(man, mu, cov, v, 1e-4, method=method)
        assert (o["status"] == 0).all() and np.array_equal(o["cov"], cov) and np.array_equal(o["mu"], mu)
        lam, _ = corr_eigs(cov, v)
        assert np.abs(o["eig_min"] - lam[:, 0]).max() <= 1e-12 and np.abs(o["eig_max"] - lam[:, -1]).max() <= 1e-12
        assert (o["eig_min"] >= 1e-4).all()


def test_indefinite_block_in_the_identity_has_its_closed_form():
    """C = I_12 with the (2, 7) block [[1, r], [r, 1]], r = 1.2: eigenvalues 1 + r, 1 - r = -0.2 on (e_2 -+ e_7) / sqrt 2.  The
    repair lifts -0.2 to eps: C'_27 = r - (eps + 0.2) / 2, C'_22 = C'_77 = 1 + (eps + 0.2) / 2; the sigmas scale it back."""
    D, r, eps = 12, 1.2, 1e-6
    s = np.linspace(0.5, 3.0, D)
    C = np.eye(D)
    C[2, 7] = C[7, 2] = r
    cov = (C * np.outer(s, s))[None]
    mu = np.zeros((1, 13))
    mu[0, 6] = 1.0
    for method in ("eigh", "jacobi"):
        o = cr.condition(on.POSE, mu, cov, np.full(D, 1e-9), eps, method=method)
        assert o["status"][0] == cr.ST_REPAIRED
        assert abs(o["eig_min"][0] - (1.0 - r)) <= 1e-14 and abs(o["eig_max"][0] - (1.0 + r)) <= 1e-14
        want = np.eye(D)
        h = 0.5 * (eps - (1.0 - r))
        want[2, 7] = want[7, 2] = r - h
        want[2, 2] = want[7, 7] = 1.0 + h
        got = o["cov"][0] / np.outer(s, s)
        assert np.abs(got - want).max() <= 1e-14, np.abs(got - want).max()
        assert np.array_equal(o["cov"][0], o["cov"][0].T)


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("eps,dtype", [(0.05, np.float64), (1e-10, np.float64), (1e-4, np.float32)])
def test_repair_recovers_and_is_idempotent(model, eps, dtype):
    """eps = 0.05 pins `every eigenvalue of C' >= eps (1 - 1e-12)` as it stands: the eigenvalues of a matrix with entries of order
    one carry an absolute error of about D u = 1.4e-15 (the rounding of C' and eigvalsh's own backward error), so a RELATIVE
    1e-12 of eps can only be asked where eps 1e-12 is well above that.  The operational floors (1e-10 for fp64 storage, 1e-4 for
    fp32) are held to the same bound with that absolute error, 4 D u lambda_max, granted."""
    man, mu, cov, v, quarter = batch(model, eps, dtype)
    lam, raised = corr_eigs(cov, v)
    # the quarters are what they claim; the verdict is unambiguous for every filter
    assert ((lam[:, 0] <= eps / 4) | (lam[:, 0] >= eps)).all()
    assert (lam[quarter == 0, 0] >= eps).all() and not raised[quarter != 3].any() and raised[quarter == 3].all()
    assert (np.abs(lam[quarter == 1, 0] + 1e-3) <= 1e-4).all() and (lam[quarter == 1, 1] >= eps).all()
    assert (lam[quarter == 2, 1] < 0).all() and (lam[quarter == 2, 0] > -0.35).all() and (lam[quarter == 2, 2] >= eps).all()
    assert (np.abs(lam[quarter == 3, 0] / (eps / 8) - 1.0) <= 0.25).all()
    L, ok = on.cholesky_lower(cov)
    assert not ok[quarter == 1].any() and not ok[quarter == 2].any() and ok[quarter == 0].all()
    outs = {m: cr.condition(man, mu, cov, v, eps, method=m) for m in ("eigh", "jacobi")}
    for m, o in outs.items():
        assert np.array_equal(o["status"], np.where(quarter == 0, 0, cr.ST_REPAIRED)), m
        assert np.array_equal(o["cov"][quarter == 0], cov[quarter == 0]) and np.array_equal(o["mu"], mu)
        assert np.array_equal(o["cov"], np.swapaxes(o["cov"], 1, 2))
        assert np.abs(o["eig_min"] - lam[:, 0]).max() <= 1e-12 and np.abs(o["eig_max"] - lam[:, -1]).max() <= 1e-12
        # every eigenvalue of C' (in the sigmas the call used) is at least eps
        C, s, d, _ = cr.correlation(cov, v)
        Cn = o["cov"] / (s[:, :, None] * s[:, None, :])
        slack = 0.0 if eps >= 0.01 else 4.0 * man.D * cr.U64 * lam[:, -1].max()
        assert (np.linalg.eigvalsh(Cn)[:, 0] >= eps * (1.0 - 1e-12) - slack).all()
        assert (np.einsum("bii->bi", o["cov"]) >= v).all()
        L, ok = on.cholesky_lower(o["cov"])
        assert ok.all(), m
        # the second application: healthy, nothing moves
        again = cr.condition(man, o["mu"], o["cov"], v, eps, method=m)
        assert (again["status"] == 0).all() and np.array_equal(again["cov"], o["cov"]) and np.array_equal(again["mu"], o["mu"])
        assert (again["eig_min"] >= 0.6 * eps).all()
    # the two eigensolvers agree on C'
    C, s, d, _ = cr.correlation(cov, v)
    diff = np.abs(outs["eigh"]["cov"] - outs["jacobi"]["cov"]) / (s[:, :, None] * s[:, None, :])
    print(f"condition reference {model} eps={eps:g}: max |C'_eigh - C'_jacobi| = {diff.max():.3e}, sweeps <= {outs['jacobi']['sweeps'].max()}")
    assert diff.max() <= 1e-12 and outs["jacobi"]["sweeps"].max() <= 8


def test_jacobi_against_eigh_and_its_cap():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((64, 13, 13))
    C = A @ np.swapaxes(A, 1, 2)
    lam, V, conv, sweeps = cr.jacobi_eig(C / np.trace(C, axis1=1, axis2=2)[:, None, None] * 13.0)
    Cn = C / np.trace(C, axis1=1, axis2=2)[:, None, None] * 13.0
    assert conv.all() and sweeps.max() <= 10
    assert np.abs(np.sort(lam, axis=1) - np.linalg.eigvalsh(Cn)).max() <= 1e-13
    assert np.abs(np.einsum("bik,bk,bjk->bij", V, lam, V) - Cn).max() <= 1e-13
    assert np.abs(np.swapaxes(V, 1, 2) @ V - np.eye(13)).max() <= 1e-14
    # one sweep is not enough: not converged, nothing published
    lam1, V1, conv1, _ = cr.jacobi_eig(Cn, max_sweeps=1)
    assert not conv1.any() and np.isnan(lam1).all()
    # a diagonal matrix is finished before the first sweep; entries at the rounding level are not rotated
    E = np.eye(12) + 1e-17 * (np.ones((12, 12)) - np.eye(12))
    lam, V, conv, sweeps = cr.jacobi_eig(E[None])
    assert conv.all() and sweeps[0] == 0 and np.array_equal(V[0], np.eye(12))


def test_variance_floor():
    """step 2: a diagonal below the floor is raised (and the filter is deficient whatever its eigenvalues), one at the floor is
    not; the repaired diagonal is never below the floor"""
    mu, cov, _ = states("pose")
    mu, cov = mu[:8], cov[:8].copy()
    v = np.einsum("bii->bi", cov).min(axis=0) * 0.5
    cov[1, 4, 4] = v[4]                        # at the floor: stays
    cov[2, 4, 4] = np.nextafter(v[4], 0.0)     # one ulp below: raised
    cov[3, 9, 9] = -1.0                        # negative: raised
    o = cr.condition(on.POSE, mu, cov, v, 1e-10)
    assert np.array_equal(o["status"], np.array([0, 0, cr.ST_REPAIRED, cr.ST_REPAIRED, 0, 0, 0, 0], dtype=np.uint32))
    assert np.array_equal(o["cov"][[0, 1, 4]], cov[[0, 1, 4]])
    assert o["cov"][2, 4, 4] >= v[4] and o["cov"][3, 9, 9] >= v[9] and abs(o["cov"][2, 4, 4] / v[4] - 1.0) <= 1e-12
    again = cr.condition(on.POSE, o["mu"], o["cov"], v, 1e-10)
    assert (again["status"] == 0).all() and np.array_equal(again["cov"], o["cov"])
    # a bad floor: every selected filter, nothing moves
    for bad in (0.0, -1.0, np.nan, np.inf):
        vb = v.copy()
        vb[7] = bad
        sel = np.ones(8, dtype=np.uint8)
        sel[5] = 0
        o = cr.condition(on.POSE, mu, cov, vb, 1e-10, select=sel)
        assert np.array_equal(o["status"], np.where(sel != 0, on.ST_ERR_NONFINITE_MEAS, on.ST_INACTIVE))
        assert np.array_equal(o["cov"], cov) and np.isnan(o["eig_min"]).all()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_quaternion_renormalisation(model):
    man = man_of(model)
    mu, cov, _ = states(model)
    mu, cov = mu[:8].copy(), cov[:8]
    Q = cr.quat_offset(man)
    assert Q == (3 if model == "pose" else 0)
    v = np.einsum("bii->bi", cov).min(axis=0) * 0.5
    unit = mu[:, Q:Q + 4] / np.linalg.norm(mu[:, Q:Q + 4], axis=1, keepdims=True)
    mu[:, Q:Q + 4] = unit
    mu[1, Q:Q + 4] *= 1.0 + 1e-3
    mu[2, Q:Q + 4] *= 0.5
    mu[3, Q:Q + 4] = 0.0
    mu[4, Q + 1] = np.nan
    o = cr.condition(man, mu, cov, v, 1e-10, renormalize=True)
    assert np.array_equal(o["status"], np.array([0, cr.ST_REPAIRED, cr.ST_REPAIRED, on.ST_ERR_CHOLESKY, on.ST_ERR_CHOLESKY, 0, 0, 0], dtype=np.uint32))
    assert np.array_equal(o["mu"][[0, 3, 5, 6, 7]], mu[[0, 3, 5, 6, 7]]) and np.array_equal(o["mu"][4], mu[4], equal_nan=True)
    assert np.abs(o["mu"][1:3, Q:Q + 4] - unit[1:3]).max() <= 4e-16   # the direction is kept
    assert np.abs(np.sum(o["mu"][1:3, Q:Q + 4] ** 2, axis=1) - 1.0).max() <= 8.0 * cr.U64   # inside the rule: idempotent
    again = cr.condition(man, o["mu"][:3], cov[:3], v, 1e-10, renormalize=True)
    assert (again["status"] == 0).all() and np.array_equal(again["mu"], o["mu"][:3])
    others = np.ones(man.S, bool)
    others[Q:Q + 4] = False
    assert np.array_equal(o["mu"][:, others], mu[:, others]) and np.array_equal(o["cov"], cov)
    assert np.isnan(o["eig_min"][3:5]).all() and np.isfinite(o["eig_min"][[0, 1, 2, 5]]).all()
    # the flag off: the mean is not looked at
    off = cr.condition(man, mu, cov, v, 1e-10)
    assert (off["status"] == 0).all() and np.array_equal(off["mu"], mu, equal_nan=True)
    # a quaternion rounded to fp32 is unit to the rounding of fp32 storage, not of fp64
    m32 = mu[:1].copy()
    m32[0, Q:Q + 4] = unit[0].astype(np.float32)
    assert cr.condition(man, m32, cov[:1], v, 1e-10, renormalize=True, u_storage=cr.U32)["status"][0] == 0
    assert cr.condition(man, m32, cov[:1], v, 1e-10, renormalize=True, u_storage=cr.U64)["status"][0] == cr.ST_REPAIRED


def test_status_rules():
    mu, cov, _ = states("orient")
    mu, cov = mu[:8], cov[:8].copy()
    v = np.einsum("bii->bi", cov).min(axis=0) * 0.5
    init = np.ones(8, bool)
    init[1] = False
    sel = np.ones(8, dtype=np.uint8)
    sel[2] = 0
    cov[3, 12, 0] = np.nan       # the lower triangle: read
    cov[4, 0, 12] = np.inf       # the upper triangle: never read
    cov[1, 5, 5] = np.nan        # an uninitialised filter is not looked at
    o = cr.condition(on.ORIENT, mu, cov, v, 1e-10, select=sel, initialised=init)
    assert np.array_equal(o["status"], np.array([0, on.ST_UNINITIALISED, on.ST_INACTIVE, on.ST_ERR_CHOLESKY, 0, 0, 0, 0], dtype=np.uint32))
    assert np.array_equal(o["cov"], cov, equal_nan=True) and np.array_equal(o["mu"], mu)
    assert np.isnan(o["eig_min"][1:4]).all() and np.isfinite(o["eig_min"][[0, 4, 5]]).all()
