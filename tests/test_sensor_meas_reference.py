"""Pins for tests/sensor_meas_reference.py, the NumPy statement of the sensor-frame measurements (include/ukf_batch.h) the
GPU tests compare with: the degenerate mount reproduces the existing models bit for bit, a sample that equals h(mu) barely
moves the mean, a far beacon's range update is the EKF's through the analytic Jacobian up to the analytic remainder, and
every h agrees with an independent matrix-form evaluation."""
import numpy as np
import pytest

import sensor_meas_reference as sr
from oracle import ukf_numpy as on
from sensor_meas_cases import N, mounts, states


# ---------------------------------------------------------------------------------------------- the degenerate mount
def test_degenerate_mount_is_the_existing_model_bit_for_bit():
    """r = 0, qs = (0, 0, 0, 1): POSE_POSITION = pose_update(MEAS_POS3), POSE_VELOCITY = MEAS_VEL3, ORIENT_VELOCITY =
    orient_update -- the same bits in mean, covariance and status"""
    rng = np.random.default_rng(3)
    Q = np.broadcast_to(0.05 ** 2 * np.eye(3), (N, 3, 3)).copy()
    mu, cov, _ = states("pose")
    for sid, mid, sl in ((sr.POSE_POSITION, on.MEAS_POS3, slice(0, 3)), (sr.POSE_VELOCITY, on.MEAS_VEL3, slice(7, 10))):
        z = mu[:, sl] + 0.05 * rng.standard_normal((N, 3))
        got = sr.update_sensor(on.POSE, mu, cov, sid, z, Q, sr.IDENTITY_MOUNT, np.zeros(3))
        m2, c2, st = on.pose_update(mu, cov, mid, z, Q)
        assert np.array_equal(got["mu"], m2) and np.array_equal(got["cov"], c2) and np.array_equal(got["status"], st)
        assert (st == 0).all() and not np.array_equal(m2, mu)
    mu, cov, gyro = states("orient")
    z = on.quat_rotate(on.quat_inverse(mu[:, 0:4]), mu[:, 4:7]) + 0.05 * rng.standard_normal((N, 3))
    got = sr.update_sensor(on.ORIENT, mu, cov, sr.ORIENT_VELOCITY, z, Q, sr.IDENTITY_MOUNT, np.zeros(3), gyro)
    m2, c2, st = on.orient_update(mu, cov, z, Q)
    assert np.array_equal(got["mu"], m2) and np.array_equal(got["cov"], c2) and np.array_equal(got["status"], st)
    assert (st == 0).all() and not np.array_equal(m2, mu)


# --------------------------------------------------------------------------------------------- a sample that is h(mu)
def test_point_sample_at_h_of_mu_moves_the_mean_at_rounding_level():
    """POSE_POINT with z = h(mu) exactly.  nu = h(mu) - z-bar, and z-bar is the mean of an odd-symmetric sigma set mapped
    through h: the first-order terms cancel and what is left is h's curvature times Sigma (~ theta^2 |b - p| / 2).  With the
    synthetic covariance as it is (sigma_theta ~ 0.05 rad, beacons 15 ... 80 m away) that term is a few centimetres and moves the
    mean by 5 % of a standard deviation: NOT rounding.  It falls with Sigma; at 1e-12 Sigma the change is rounding alone."""
    mu, cov, _ = states("pose")
    mount, rng = mounts(N)
    d = rng.standard_normal((N, 3))
    b = mu[:, 0:3] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(15.0, 80.0, (N, 1))
    z = sr.h(sr.POSE_POINT, mu, mount, b)
    moved = {}
    for scale in (1.0, 1e-12):
        got = sr.update_sensor(on.POSE, mu, scale * cov, sr.POSE_POINT, z, np.broadcast_to(scale * 0.05 ** 2 * np.eye(3), (N, 3, 3)),
                               mount, b)
        assert (got["status"] == 0).all()
        moved[scale] = np.abs(on.POSE.boxminus(got["mu"], mu))
    rel = (moved[1.0] / np.sqrt(np.einsum("bii->bi", cov))).max()
    print(f"max |mu' (-) mu| / sigma at Sigma = {rel:.3e}; max |mu' (-) mu| at 1e-12 Sigma = {moved[1e-12].max():.3e}")
    # observed on the CPU: 5.10e-2 standard deviations (the curvature term); x 10
    assert rel <= 5.1e-1
    # observed on the CPU: 1.87e-14 (metres, radians, ...) -- a few ulp of the 80 m that h subtracts; x 10
    assert moved[1e-12].max() <= 1.9e-13


# ------------------------------------------------------------------------------------- a far beacon: the EKF's update
def test_range_of_a_far_beacon_is_the_ekf_update_to_first_order():
    """h = |u|, u = (p - b) + R(q) r.  Per sigma point X_i = mu (+) x_i (x_i = 0, +-L col j; c = the position part of x_i, th
    its rotation part) the analytic remainder against the first-order model J x_i, J = u^T [I, -R(q) [r]x, 0, 0] / |u|, is
        |h(X_i) - h(mu) - J x_i| <= e_i = |du|^2 / (2 (rho - |du|)) + (|th|^2 / 2 + |th|^3 / 6) |r|,
        |du| <= |c| + (|th| + |th|^2 / 2 + |th|^3 / 6) |r|,  rho = |u(mu)|
    (second-order Taylor of the norm, whose Hessian is bounded by 1 / |u|, and of the rotation's exponential).  With
    e-bar = mean e_i:  |z-bar - h(mu)| <= e-bar, and S - (J Sigma J^T + Q) = sum_i (J x_i) f_i + 1/2 sum f_i^2 with
    |f_i| <= e_i + e-bar; C - Sigma J^T = sum_j (L col j) (e_j+ - e_j-) / 2.  Beacons at 20 m, sigma ~ 0.1 m / 0.05 rad, lever
    arms up to 1.7 m: the second-order term is visible (orders above rounding) and bounded (S within 25 %, z-bar within a
    centimetre; the lever arm's theta^2 |r| / 2 dominates the bound, the beacon's |du|^2 / 2 rho follows)."""
    mu, cov, _ = states("pose")
    mount, rng = mounts(N)
    d = rng.standard_normal((N, 3))
    b = mu[:, 0:3] + 20.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    Q = np.zeros((N, 3, 3))
    Q[:, 0, 0] = 0.05 ** 2
    r = mount[:, 0:3]
    q = mu[:, 3:7]
    u = (mu[:, 0:3] - b) + on.quat_rotate(q, r)
    rho = np.linalg.norm(u, axis=1)
    z = np.zeros((N, 3))
    z[:, 0] = rho + 0.05 * rng.standard_normal(N)
    got = sr.update_sensor(on.POSE, mu, cov, sr.POSE_RANGE, z, Q, mount, b)
    assert (got["status"] == 0).all()
    # the analytic Jacobian: d u = d p + R(q) (th x r) = d p - R(q) [r]x th
    R = on.quat_to_matrix(q)
    rx = np.zeros((N, 3, 3))
    rx[:, 0, 1], rx[:, 0, 2], rx[:, 1, 0], rx[:, 1, 2], rx[:, 2, 0], rx[:, 2, 1] = -r[:, 2], r[:, 1], r[:, 2], -r[:, 0], -r[:, 1], r[:, 0]
    uh = u / rho[:, None]
    J = np.zeros((N, 12))
    J[:, 0:3] = uh
    J[:, 3:6] = -np.einsum("bi,bij->bj", uh, R @ rx)
    L, ok = on.cholesky_lower(cov)
    assert ok.all()
    x = np.concatenate([L, -L], axis=2).swapaxes(1, 2)   # [N, 24, 12]: +-L col j
    rn = np.linalg.norm(r, axis=1)[:, None]
    c, th = np.linalg.norm(x[:, :, 0:3], axis=2), np.linalg.norm(x[:, :, 3:6], axis=2)
    du = c + (th + th ** 2 / 2 + th ** 3 / 6) * rn
    e = du ** 2 / (2.0 * (rho[:, None] - du)) + (th ** 2 / 2 + th ** 3 / 6) * rn
    ebar = e.sum(axis=1) / 25.0
    Jx = np.abs(np.einsum("bk,bik->bi", J, x))
    f = e + ebar[:, None]
    bound_S = (Jx * f).sum(axis=1) + 0.5 * ((f ** 2).sum(axis=1) + ebar ** 2)
    S_ekf = np.einsum("bi,bij,bj->b", J, cov, J) + Q[:, 0, 0]
    dz, dS = np.abs(got["z_pred"][:, 0] - rho), np.abs(got["S"][:, 0, 0] - S_ekf)
    print(f"max |z-bar - h(mu)| = {dz.max():.3e} (bound {ebar.max():.3e}); max |S - S_ekf| / S = {(dS / S_ekf).max():.3e} "
          f"(bound {(bound_S / S_ekf).max():.3e})")
    slack = 1e-12
    assert (dz <= ebar + slack).all() and (dS <= bound_S + slack).all()
    assert dz.max() > 1e-6 and (dS / S_ekf).max() > 1e-6          # visible: not rounding
    assert (bound_S / S_ekf).max() < 0.25 and ebar.max() < 0.01   # bounded: a correction, not another update
    # the update itself against the EKF's, mu' = mu (+) K nu with K = Sigma J^T / S_ekf, nu = z - h(mu): the committed mean IS
    # mu (+) C nu / S up to rounding (applyDelta re-samples around it), with C, nu and S inside the intervals above, and
    # |x y / s - x0 y0 / s0| <= (|x0| + bx) (|y0| + by) / (s0 - bs) - |x0| |y0| / s0
    C_ekf = np.einsum("bij,bj->bi", cov, J)
    nu = z[:, 0] - rho
    delta_ekf = C_ekf * (nu / S_ekf)[:, None]
    delta = on.POSE.boxminus(got["mu"], mu)
    bound_C = 0.5 * np.einsum("bik,bi->bk", np.abs(x), e)
    bound_d = ((np.abs(C_ekf) + bound_C) * ((np.abs(nu) + ebar) / (S_ekf - bound_S))[:, None]
               - np.abs(C_ekf) * (np.abs(nu) / S_ekf)[:, None])
    dd = np.abs(delta - delta_ekf)
    print(f"max |delta - delta_ekf| = {dd.max():.3e} (largest bound {bound_d.max():.3e})")
    assert (dd <= bound_d + slack).all()
    assert dd.max() > 1e-6


# ------------------------------------------------------------------------------------------- h against matrix forms
@pytest.mark.parametrize("mid", list(range(8)))
def test_h_against_matrix_form(mid):
    n = 257
    model = "pose" if mid <= 4 else "orient"
    mu, _, gyro = states(model)
    mu = mu[:n]
    mount, rng = mounts(n, seed=17 + mid)
    b = 30.0 * rng.standard_normal((n, 3))
    gyro = rng.standard_normal((n, 3)) if gyro is None else gyro[:n] + rng.standard_normal((n, 3))
    r, Rs = mount[:, 0:3], on.quat_to_matrix(mount[:, 3:7])
    mv = lambda M, x: np.einsum("bij,bj->bi", M, x)
    tv = lambda M, x: np.einsum("bji,bj->bi", M, x)
    if model == "pose":
        p, R, v, w = mu[:, 0:3], on.quat_to_matrix(mu[:, 3:7]), mu[:, 7:10], mu[:, 10:13]
        want = {0: lambda: p + mv(R, r),
                1: lambda: np.linalg.norm(p + mv(R, r) - b, axis=1, keepdims=True),
                2: lambda: tv(Rs, tv(R, b - p) - r),
                3: lambda: tv(Rs, v + np.cross(w, r)),
                4: lambda: mv(R, v)}[mid]()
    else:
        R, v, bg, ba, g = on.quat_to_matrix(mu[:, 0:4]), mu[:, 4:7], mu[:, 7:10], mu[:, 10:13], mu[:, 13]
        e3 = np.zeros((n, 3))
        e3[:, 2] = g
        want = {5: lambda: tv(Rs, tv(R, v) + np.cross(gyro - bg, r)),
                6: lambda: tv(Rs, tv(R, b)),
                7: lambda: tv(R, e3) + ba}[mid]()
    got = sr.h(mid, mu, mount, b, gyro)
    assert got.shape == (n, sr.meas_dim(mid))
    # quaternion and matrix forms of a rotation differ by a few ulp of the vector's length (<= 100 here)
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()
    assert np.abs(want).max() > 0.1


def test_unused_inputs_and_status_rules():
    """NaN in an entry a model does not read changes nothing; in one it reads: ERR_NONFINITE_MEAS, the state kept; ids of the
    other engine and negative ids: INACTIVE"""
    n = 16
    mu, cov, _ = states("pose")
    mu, cov = mu[:n], cov[:n]
    mount, rng = mounts(n)
    b = mu[:, 0:3] + 30.0
    Q = np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)).copy()
    ids = (np.arange(n) % 7 - 1).astype(np.int64)   # -1, 0 ... 4, 5 (OrientationState's)
    z = np.zeros((n, 3))
    for mid in sr.POSE_IDS:
        i = ids == mid
        z[i, :sr.meas_dim(mid)] = sr.h(mid, mu[i], mount[i], b[i]) + 0.01
    clean = sr.update_sensor(on.POSE, mu, cov, ids, z, Q, mount, b)
    assert np.array_equal(clean["status"], np.where((ids < 0) | (ids > 4), on.ST_INACTIVE, 0))
    z2, Q2, m2, b2 = z.copy(), Q.copy(), mount.copy(), b.copy()
    for i in range(n):
        uz, uq, um, up = sr.used_inputs(int(ids[i])) if 0 <= ids[i] <= 4 else (np.zeros(3, bool), np.zeros((3, 3), bool), np.zeros(7, bool), np.zeros(3, bool))
        z2[i, ~uz], m2[i, ~um], b2[i, ~up] = np.nan, np.nan, np.nan
        Q2[i][~uq] = np.nan
    dirty = sr.update_sensor(on.POSE, mu, cov, ids, z2, Q2, m2, b2)
    for k in clean:
        assert np.array_equal(clean[k], dirty[k], equal_nan=True), k
    z3 = z.copy()
    z3[1, 0] = np.nan
    bad = sr.update_sensor(on.POSE, mu, cov, ids, z3, Q, mount, b)
    assert bad["status"][1] == on.ST_ERR_NONFINITE_MEAS and np.array_equal(bad["mu"][1], mu[1]) and np.isnan(bad["maha"][1])


# --------------------------------------------------------------------------- the kernel's arithmetic, restated in NumPy
def kernel_form(man, mu, cov, mid, z, Q, mount, point, gyro):
    """What ukf_sensor_meas.hpp computes, step by step: the three-dimensional embedding of m = 1, the mean and
    the deltas relative to Z_0, S from the half sums u and half
    differences w of a lane's two deltas, C = sum_j (L col j) W_j^T, the 3 x 3 factor in pivots and reciprocal roots, Y = C Ls^-T,
    y = Ls^-1 nu, Sigma~ = Sigma - Y Y^T, delta = Y y, ln det S from the pivots."""
    B, D, m = mu.shape[0], man.D, sr.meas_dim(mid)
    L, ok = on.cholesky_lower(cov)
    X, _ = on.sigma_points(man, mu, cov)
    Z = np.zeros((B, 2 * D + 1, 3))
    Z[..., :m] = sr.h(mid, X, mount[:, None, :], point[:, None, :], gyro[:, None, :])
    z0 = Z[:, 0].copy()
    Zs = Z - z0[:, None, :]   # coordinates whose origin is Z_0: the iterate is small whatever the beacon's distance
    ref = np.zeros((B, 3))
    for _ in range(2):   # on a vector space the mean moves once and confirms
        ref = ref + (Zs - ref[:, None, :]).sum(axis=1) / (2 * D + 1)
    dp, dm, d0 = Zs[:, 1::2] - ref[:, None, :], Zs[:, 2::2] - ref[:, None, :], -ref
    u, w = 0.5 * (dp + dm), 0.5 * (dp - dm)
    S = np.einsum("bjr,bjc->brc", u, u) + np.einsum("bjr,bjc->brc", w, w) + 0.5 * d0[:, :, None] * d0[:, None, :]
    pad = np.eye(3)
    pad[:m, :m] = 0.0
    Qe = np.zeros((B, 3, 3))
    Qe[:, :m, :m] = Q[:, :m, :m]
    keep = np.zeros((3, 3))
    keep[:m, :m] = 1.0
    S = S * keep + Qe + pad
    nu = np.zeros((B, 3))
    nu[:, :m] = (z[:, :m] - z0[:, :m]) - ref[:, :m]
    ref = z0 + ref
    C = np.einsum("blj,bjc->blc", L, w)
    d0_, t10, t20 = S[:, 0, 0], S[:, 1, 0] / S[:, 0, 0], S[:, 2, 0] / S[:, 0, 0]
    d1 = S[:, 1, 1] - t10 * S[:, 1, 0]
    a21 = S[:, 2, 1] - t20 * S[:, 1, 0]
    d2 = S[:, 2, 2] - t20 * S[:, 2, 0] - a21 / d1 * a21
    rs = [1.0 / np.sqrt(d0_), 1.0 / np.sqrt(d1), 1.0 / np.sqrt(d2)]
    l10, l20, l21 = S[:, 1, 0] * rs[0], S[:, 2, 0] * rs[0], a21 * rs[1]

    def solve(c):
        y0 = c[..., 0] * rs[0][(...,) + (None,) * (c.ndim - 2)]
        y1 = (c[..., 1] - l10[(...,) + (None,) * (c.ndim - 2)] * y0) * rs[1][(...,) + (None,) * (c.ndim - 2)]
        y2 = (c[..., 2] - l20[(...,) + (None,) * (c.ndim - 2)] * y0 - l21[(...,) + (None,) * (c.ndim - 2)] * y1) * rs[2][(...,) + (None,) * (c.ndim - 2)]
        return np.stack([y0, y1, y2], axis=-1)

    Y, y = solve(C), solve(nu)
    maha = np.sum(y * y, axis=1)
    lndet = np.log(d0_) + np.log(d1) + np.log(d2)
    sig2 = cov - Y @ np.swapaxes(Y, 1, 2)
    m2, C2, ok2 = on.apply_delta(man, mu, sig2, np.einsum("blk,bk->bl", Y, y))
    assert ok.all() and ok2.all()
    return {"mu": m2, "cov": C2, "z_pred": ref * keep[0] if m == 1 else ref, "S": S * keep, "innov": nu, "maha": maha,
            "loglik": -0.5 * (maha + lndet + m * sr.LN_2PI)}


@pytest.mark.parametrize("mid", list(range(8)))
def test_kernel_form_agrees_with_the_reference(mid):
    n = 257
    model = "pose" if mid <= 4 else "orient"
    man = on.POSE if model == "pose" else on.ORIENT
    mu, cov, gyro = states(model)
    mu, cov = mu[:n], cov[:n]
    mount, rng = mounts(n)
    d = rng.standard_normal((n, 3))
    away = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(15.0, 80.0, (n, 1))
    point = mu[:, 0:3] + away if model == "pose" else away
    gyro = np.zeros((n, 3)) if gyro is None else gyro[:n]
    m = sr.meas_dim(mid)
    z = np.zeros((n, 3))
    z[:, :m] = sr.h(mid, mu, mount, point, gyro) + 0.05 * rng.standard_normal((n, m))
    Q = np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3))
    ref = sr.update_sensor(man, mu, cov, mid, z, Q, mount, point, gyro)
    assert (ref["status"] == 0).all()
    got = kernel_form(man, mu, cov, mid, z, Q, mount, point, gyro)
    worst = max(float(np.max(np.abs(got[k] - ref[k]) / (1.0 + np.abs(ref[k])))) for k in got)
    print(f"{sr.NAMES[mid]}: kernel form against the reference, max scaled difference {worst:.3e}")
    # two float64 evaluations of the same update in another order of operations: a few hundred eps times the condition of S (up to
    # ~ 1e4 here: (sigma_theta * 80 m / 0.05)^2) stays below 1e-11; the fp64 device gate is 1e-9
    assert worst <= 1e-11
