"""NumPy float64 statement of the sensor-frame association of include/ukf_batch.h ("sensor-frame association"), made of
sensor_meas_reference.update_sensor alone: one SCORING call per candidate, the best rule of ukfb_innovation_dev, the statuses
of the header, and one COMMITTING call with the chosen candidates.  A helper, not collected;
tests/test_associate_reference.py pins it.

z [K, B, 3]; point [3] / [B, 3] (shared-h mode) or, with point_per_candidate, [K, B, 3] (per-hypothesis mode: candidate k pairs
z[k] with point[k]).  H = K per hypothesis, else 1.

The scoring calls run with gate_chi2 = 0, a gate only an innovation of exactly zero passes: update_sensor then writes the
scores of every candidate whose S is positive definite and judges no Sigma~ -- the header's rule, "a candidate whose own S
fails scores NaN".  Sigma~ is judged where the header says, in the accepted update: the committing call gets z[best] (and
point[best]) with no gate (the candidate is inside it already) and model id -1 for the filters without a best candidate."""
import numpy as np

import sensor_meas_reference as sr
from oracle import ukf_numpy as on

FAILED = on.ST_UNINITIALISED | on.ST_INACTIVE | on.ST_ERR_NONFINITE_MEAS | on.ST_ERR_CHOLESKY


def pick_best(maha, gate_chi2):
    """maha [K, B] (NaN: not scored) -> (best [B] int32, n_gated [B] int32): the smallest finite d^2, with gate_chi2 >= 0 only
    among d^2 <= gate_chi2; equal d^2: the lower index; -1: none"""
    fin = np.isfinite(maha)
    inside = fin if gate_chi2 < 0 else fin & (np.where(fin, maha, np.inf) <= gate_chi2)
    key = np.where(inside, maha, np.inf)
    best = np.argmin(key, axis=0).astype(np.int32)   # (argmin returns the first of equal minima)
    best[~inside.any(axis=0)] = -1
    return best, inside.sum(axis=0).astype(np.int32)


def associate_sensor(man, mu, cov, models, z, Q, mount, point, gyro=None, point_per_candidate=False, gate_chi2=-1.0,
                     initialised=None, commit=True, tol=on.MEAN_TOL, max_it=on.MEAN_MAX_IT):
    """-> dict(mu, cov, z_pred [H, B, 3], S [H, B, 3, 3], innov [K, B, 3], maha [K, B], loglik [K, B], best [B], n_gated [B],
    status [B])"""
    z = np.asarray(z, dtype=np.float64)
    K, B = z.shape[0], z.shape[1]
    H = K if point_per_candidate else 1
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    point = np.asarray(point, dtype=np.float64)
    pts = point if point_per_candidate else np.broadcast_to(point, (1, B, 3))
    assert pts.shape == (H, B, 3)
    hyp = (lambda k: k) if point_per_candidate else (lambda k: 0)
    kw = dict(initialised=initialised, tol=tol, max_it=max_it)
    per = [sr.update_sensor(man, mu, cov, models, z[k], Q, mount, pts[hyp(k)], gyro, gate_chi2=0.0, **kw) for k in range(K)]
    stack = lambda key: np.stack([p[key] for p in per])   # noqa: E731
    st = stack("status")                                                        # [K, B]
    dead = (st[0] & (on.ST_UNINITIALISED | on.ST_INACTIVE)) != 0                # the same for every candidate
    absent = (st & on.ST_ERR_NONFINITE_MEAS) != 0
    scored = ~dead[None] & ~absent & ((st & on.ST_ERR_CHOLESKY) == 0)
    o = {"innov": stack("innov"), "maha": stack("maha"), "loglik": stack("loglik")}
    if point_per_candidate:
        o["z_pred"], o["S"] = stack("z_pred"), stack("S")
    else:   # one hypothesis: z-bar and S do not depend on z; those of the first scored candidate (NaN when there is none)
        src = np.argmax(scored, axis=0)
        o["z_pred"], o["S"] = stack("z_pred")[src, np.arange(B)][None], stack("S")[src, np.arange(B)][None]
    best, n_gated = pick_best(np.where(scored, o["maha"], np.nan), gate_chi2)
    status = np.zeros(B, dtype=np.uint32)
    status[dead] = st[0][dead]
    none_present = ~dead & absent.all(axis=0)
    status[none_present] = on.ST_ERR_NONFINITE_MEAS
    live = ~dead & ~none_present
    # (Sigma failing fails every present candidate: it is part of "no present candidate has a positive-definite S")
    status[live & ~scored.any(axis=0)] = on.ST_ERR_CHOLESKY
    # ---- the accepted update
    sel = np.maximum(best, 0)
    upd = sr.update_sensor(man, mu, cov, np.where((status == 0) & (best >= 0), models, -1), z[sel, np.arange(B)], Q, mount,
                           pts[sel if point_per_candidate else 0, np.arange(B)], gyro, gate_chi2=-1.0, **kw)
    acc = (status == 0) & (best >= 0)
    status[acc & ((upd["status"] & on.ST_ERR_CHOLESKY) != 0)] = on.ST_ERR_CHOLESKY
    ok = live & (status == 0)
    noconv = (~absent & ((st & on.ST_WARN_MEAN_NOCONV) != 0)).any(axis=0)
    status[ok & noconv] |= on.ST_WARN_MEAN_NOCONV
    status[ok & (best < 0) & np.isfinite(np.where(scored, o["maha"], np.nan)).any(axis=0)] |= on.ST_REJECTED_GATE
    wrote = acc & ((status & FAILED) == 0)
    o["mu"], o["cov"] = mu.copy(), cov.copy()
    if commit:
        o["mu"][wrote], o["cov"][wrote] = upd["mu"][wrote], upd["cov"][wrote]
    # ---- a failed filter: NaN to its float outputs (update_sensor's padding of innov stays), -1 / 0
    failed = (status & FAILED) != 0
    best[failed], n_gated[failed] = -1, 0
    m = np.array([sr.meas_dim(int(i)) for i in models])
    lead = np.arange(3)[None, :] < m[:, None]                                    # [B, 3]: the first m entries
    for k in range(K):
        blank = failed | ~scored[k]
        o["innov"][k][blank[:, None] & (lead | dead[:, None])] = np.nan
        o["maha"][k][blank] = np.nan
        o["loglik"][k][blank] = np.nan
    for hx in range(H):
        blank = failed | (~scored[hx] if point_per_candidate else np.zeros(B, bool))
        o["z_pred"][hx][blank] = np.nan
        o["S"][hx][blank] = np.nan
    o["best"], o["n_gated"], o["status"] = best, n_gated, status
    return o


def constructed_candidates(man, mu, cov, models, z_true, Q, mount, point, gyro, K, point_per_candidate, dtype=np.float64, seed=11):
    """A constructed map with a known answer -> (z [K, B, 3], points, truth [B]): filter i's true candidate sits at index
    i % K, the others are clutter.
      * a clutter DETECTION is the true sample moved to Mahalanobis radius 6 + 3 j of the filter's own innovation covariance,
        z_true + (6 + 3 j) Ls u with S = Ls Ls^T, u a random unit vector of the measurement space and j = 1 ... K - 1 the
        clutter's rank: 9, 12, 15 ... sigma from the true sample in the metric the gate uses, whatever the shape of S.  (A
        distance set in metres instead puts clutter hundreds of sigma out along the stiff axis of an S of condition 10^3 --
        POSE_POINT, ORIENT_NAV_VECTOR -- where no gate is ever set and where a float32 d^2 is a statement about the
        conditioning of S, not about the association.)
      * a clutter LANDMARK (per-hypothesis mode, models that read the point) is the true point moved radially away from the
        filter (OrientationState: from the origin) by 3 m per rank -- 60 sigma of the measurement noise per rank in range, in
        the radial component of a fix and in the length of a nav-frame vector -- and every candidate carries the one
        detection.  Metres, not a factor: a landmark at 2.5 times 80 m sharpens the orientation update until an all-float32
        evaluation of the clutter's own commit (tests/feature_f32.py, the bound of the plain fp32 engines) no longer
        factorises, and a factor does not separate vectors of length 1.  Models that do not read the point get clutter
        detections instead.
    points: `point` itself (shared-h mode) or [K, B, 3].  Everything is rounded to the engine's storage type `dtype`.  Whether
    the construction separates the candidates is for the caller to assert on the reference's d^2 (tests/test_associate_reference.py)."""
    B = mu.shape[0]
    rng = np.random.default_rng(seed)
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    m = np.array([sr.meas_dim(int(i)) for i in models])
    reads_b = np.isin(models, sr.READS_POINT)
    point = np.broadcast_to(np.asarray(point, dtype=np.float64), (B, 3))
    S = sr.update_sensor(man, mu, cov, models, z_true, Q, mount, point, gyro, gate_chi2=0.0)["S"]
    S = np.where(np.isnan(S).any(axis=(1, 2))[:, None, None], np.eye(3), S)              # a filter without an S: any factor will do
    S = S + np.eye(3) * (np.arange(3)[None, :] >= m[:, None])[:, :, None]                # identity beyond m, where S is padded with 0
    Ls, _ = on.cholesky_lower(S)
    truth = (np.arange(B) % K).astype(np.int32)
    rank = (np.arange(K)[:, None] - truth[None, :]) % K                        # [K, B]: 0 the true one, 1 ... K - 1 the clutter
    u = rng.standard_normal((K, B, 3)) * (np.arange(3)[None, None, :] < m[None, :, None])
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    move_z = (rank > 0) & ~(point_per_candidate & reads_b)[None, :]
    z = z_true[None] + np.where(move_z, 6.0 + 3.0 * rank, 0.0)[:, :, None] * np.einsum("bij,kbj->kbi", Ls, u)
    r = lambda x: np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)   # noqa: E731
    if not point_per_candidate:
        return r(z), point, truth
    origin = mu[:, 0:3] if man is on.POSE else np.zeros((B, 3))
    arm = point - origin
    pts = point[None] + (arm / np.linalg.norm(arm, axis=1, keepdims=True))[None] * (3.0 * rank)[:, :, None]
    return r(z), r(pts), truth
