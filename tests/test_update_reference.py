"""Pins for tests/update_reference.py, the scored update every NumPy reference of a measurement feature is built on: a linear h
gives the closed-form Kalman update, and the status rules hold one by one, each produced by one constructed filter among
healthy neighbours whose rows do not change, with the scored / commit masks that go with it."""
import numpy as np

from oracle import ukf_numpy as on
from sensor_meas_cases import cycled
from update_reference import scored_update

N = 8
LN_2PI = float(np.log(2.0 * np.pi))
SEL, TSEL = [0, 1, 2, 7, 8, 9], [0, 1, 2, 6, 7, 8]   # position and velocity: stored and tangent entries
FLOATS = ("Z", "mz", "S", "innov", "d2", "logdet", "mu2", "cov2")


def pose():
    mu, cov, _ = cycled("pose", N)
    return mu, cov


# ------------------------------------------------------------------------------------------------------- a linear h: Kalman
def test_linear_h_is_the_kalman_update():
    """m = 6: position and velocity.  For a linear h the unscented statistics are exact: z-bar = H mu, S = H Sigma H^T + Q,
    C = Sigma H^T, so that K, nu, d^2 and the log-likelihood are the Kalman filter's, and the committed state is ukfom's commit
    of the Kalman result, applyDelta(mu, Sigma - K S K^T, K nu) (the mean is mu (+) K nu; on SO(3) re-sampling about the moved
    mean changes the rotation block of Sigma - K S K^T in second order, 2e-8 here, which is the update's and not an error): all
    to rounding, 1e-10."""
    mu, cov = pose()
    rng = np.random.default_rng(7)
    z = mu[:, SEL] + 0.05 * rng.standard_normal((N, 6))
    G = rng.standard_normal((N, 6, 6))
    Q = 0.05 ** 2 * (np.eye(6) + G @ np.swapaxes(G, 1, 2) / 24.0)
    got = scored_update(on.POSE, on.VECT(6), mu, cov, z, lambda X: X[..., SEL], Q, on.MEAN_TOL, on.MEAN_MAX_IT, -1.0)
    assert (got.status == 0).all() and got.commit.all() and got.scored.all() and got.ok.all()
    H = np.zeros((6, 12))
    H[np.arange(6), TSEL] = 1.0
    S = H @ cov @ H.T + Q
    K = cov @ H.T @ np.linalg.inv(S)
    nu = z - mu[:, SEL]
    mu_k, cov_k, ok = on.apply_delta(on.POSE, mu, cov - K @ S @ np.swapaxes(K, 1, 2), np.einsum("bij,bj->bi", K, nu))
    assert ok.all() and np.abs(mu_k - on.POSE.boxplus(mu, np.einsum("bij,bj->bi", K, nu))).max() <= 1e-14
    d2 = np.einsum("bi,bij,bj->b", nu, np.linalg.inv(S), nu)
    ll = -0.5 * (d2 + np.linalg.slogdet(S)[1] + 6 * LN_2PI)
    got_ll = -0.5 * (got.d2 + got.logdet + 6 * LN_2PI)
    err = {"mu": np.abs(got.mu2 - mu_k).max(), "cov": np.abs(got.cov2 - cov_k).max(), "S": np.abs(got.S - S).max(),
           "z_pred": np.abs(got.mz - mu[:, SEL]).max(), "innov": np.abs(got.innov - nu).max(),
           "maha": (np.abs(got.d2 - d2) / (1.0 + d2)).max(), "loglik": (np.abs(got_ll - ll) / (1.0 + np.abs(ll))).max()}
    print("linear h against the Kalman update: " + " ".join(f"{k}={v:.3e}" for k, v in err.items()))
    assert all(v <= 1e-10 for v in err.values()), err
    assert np.abs(got.mu2 - mu).max() > 1e-4


# ------------------------------------------------------------------------------------------------ the status rules, one by one
I = 5        # the constructed filter
FAR = 10.0   # metres by which its sample is moved where the gate is to reject it: thousands of sigmas
GATE = 1e4   # a gate every healthy filter passes (asserted) and the moved sample does not


def family():
    """position fixes with a per-filter curvature c: h(X) = p + c |p|^2.  c = 0 is linear: the mean of the sigma points'
    images is exact at the first step; c = 1 moves it by about the trace of the position block, far above the tolerance"""
    mu, cov = pose()
    rng = np.random.default_rng(3)
    z = mu[:, 0:3] + 0.05 * rng.standard_normal((N, 3))
    Q = np.broadcast_to(0.05 ** 2 * np.eye(3), (N, 3, 3)).copy()
    return mu, cov, z, Q


def run(mu, cov, z, Q, c=None, max_it=on.MEAN_MAX_IT, gate=-1.0, extra_fail=None):
    c = np.zeros(N) if c is None else c

    def h(X):
        p = X[..., 0:3]
        return p + c[:, None, None] * np.sum(p * p, axis=-1, keepdims=True)
    return scored_update(on.POSE, on.VECT(3), mu, cov, z, h, Q, on.MEAN_TOL, max_it, gate, extra_fail=extra_fail)


def bits(x):
    return x.view(np.uint64) if x.dtype == np.float64 else x


def only(got, clean, status, scored, commit, ok=True):
    """filter I has exactly `status` and the masks given; every row of every other filter is the clean run's, bit for bit"""
    rest = np.arange(N) != I
    for k in got._fields:
        assert np.array_equal(bits(getattr(got, k))[rest], bits(getattr(clean, k))[rest]), k
    assert got.status[I] == status, (got.status[I], status)
    assert (bool(got.scored[I]), bool(got.commit[I]), bool(got.ok[I])) == (scored, commit, ok)
    return got


def test_status_rules_one_by_one():
    mu, cov, z, Q = family()
    clean = run(mu, cov, z, Q)
    assert (clean.status == 0).all() and clean.scored.all() and clean.commit.all() and clean.ok.all()
    assert all(np.isfinite(getattr(clean, k)).all() for k in FLOATS)
    assert clean.d2.max() < GATE and not np.array_equal(clean.mu2, mu)
    # a gate that everyone passes changes nothing
    gated = run(mu, cov, z, Q, gate=GATE)
    assert all(np.array_equal(bits(getattr(gated, k)), bits(getattr(clean, k))) for k in clean._fields)
    far = z.copy()
    far[I] += FAR

    # Sigma indefinite: no sigma points, nothing scored, nothing committed
    bad = cov.copy()
    bad[I] = -np.eye(12)
    only(run(mu, bad, z, Q), clean, on.ST_ERR_CHOLESKY, scored=False, commit=False, ok=False)
    # ... and no REJECTED_GATE beside it, whatever the gate makes of the identity that stood in
    only(run(mu, bad, far, Q, gate=GATE), clean, on.ST_ERR_CHOLESKY, scored=False, commit=False, ok=False)

    # S indefinite
    Qn = Q.copy()
    Qn[I] = -1e6 * np.eye(3)
    only(run(mu, cov, z, Qn), clean, on.ST_ERR_CHOLESKY, scored=False, commit=False)
    only(run(mu, cov, far, Qn, gate=GATE), clean, on.ST_ERR_CHOLESKY, scored=False, commit=False)

    # the gate rejects: scored, not committed; the scores are those of the ungated call
    ungated = run(mu, cov, far, Q)
    assert ungated.status[I] == 0 and ungated.d2[I] > GATE and ungated.commit[I]
    o = only(run(mu, cov, far, Q, gate=GATE), clean, on.ST_REJECTED_GATE, scored=True, commit=False)
    assert np.array_equal(o.mu2[I], mu[I]) and np.array_equal(o.cov2[I], cov[I])
    for k in ("mz", "S", "innov", "d2", "logdet"):
        assert np.array_equal(bits(getattr(o, k))[I], bits(getattr(ungated, k))[I]), k

    # Sigma~ = Sigma - K S K^T indefinite: Q = -1/2 H Sigma H^T leaves S = 1/2 H Sigma H^T positive definite and
    # Sigma~ = Sigma - 2 Sigma H^T (H Sigma H^T)^-1 H Sigma negative on the position block.  Ungated the commit fails and
    # nothing is scored; rejected by the gate the commit is never tried: REJECTED_GATE alone, and the scores stand
    Qh = Q.copy()
    Qh[I] = -0.5 * cov[I, 0:3, 0:3]
    o = only(run(mu, cov, far, Qh), clean, on.ST_ERR_CHOLESKY, scored=False, commit=False)
    assert on.cholesky_lower(o.S[I:I + 1])[1].all()   # S itself was fine
    o = only(run(mu, cov, far, Qh, gate=GATE), clean, on.ST_REJECTED_GATE, scored=True, commit=False)
    assert np.isfinite(o.d2[I]) and o.d2[I] > GATE and np.array_equal(o.mu2[I], mu[I])

    # the mean capped: a warning; the update is scored and committed from the last iterate
    c = np.zeros(N)
    c[I] = 1.0
    zc = z + c[:, None] * np.sum(mu[:, 0:3] ** 2, axis=-1, keepdims=True)
    free = run(mu, cov, zc, Q, c=c)
    assert free.status[I] == 0
    o = only(run(mu, cov, zc, Q, c=c, max_it=1), clean, on.ST_WARN_MEAN_NOCONV, scored=True, commit=True)
    # (on R^3 the first step lands on the mean, so the capped call differs from the free one in its warning alone)
    assert not np.array_equal(o.mu2[I], mu[I]) and np.array_equal(o.mu2[I], free.mu2[I]) and np.array_equal(o.mz[I], free.mz[I])

    # extra_fail: as if S had failed, and no REJECTED_GATE beside it
    ef = np.zeros(N, bool)
    ef[I] = True
    only(run(mu, cov, z, Q, extra_fail=ef), clean, on.ST_ERR_CHOLESKY, scored=False, commit=False)
    only(run(mu, cov, far, Q, gate=GATE, extra_fail=ef), clean, on.ST_ERR_CHOLESKY, scored=False, commit=False)


def test_masks_follow_the_status():
    """scored = no ERR_CHOLESKY, commit = neither ERR_CHOLESKY nor REJECTED_GATE, and the two never coexist: over a batch in
    which every filter is one of the cases above"""
    mu, cov, z, Q = family()
    cov, z, Q = cov.copy(), z.copy(), Q.copy()
    cov[0] = -np.eye(12)
    Q[1] = -1e6 * np.eye(3)
    z[[2, 3, 4]] += FAR
    Q[3] = -0.5 * cov[3, 0:3, 0:3]
    c, ef = np.zeros(N), np.zeros(N, bool)
    c[5], ef[4], ef[6] = 1.0, True, True
    z[5] += np.sum(mu[5, 0:3] ** 2)
    o = run(mu, cov, z, Q, c=c, max_it=1, gate=GATE, extra_fail=ef)
    E, R, W = on.ST_ERR_CHOLESKY, on.ST_REJECTED_GATE, on.ST_WARN_MEAN_NOCONV
    assert o.status.tolist() == [E, E, R, R, E, W, E, 0]
    assert o.scored.tolist() == [False, False, True, True, False, True, False, True]
    assert o.commit.tolist() == [False, False, False, False, False, True, False, True]
    assert o.ok.tolist() == [False] + [True] * 7
