"""NumPy float64 statement of the fixed-interval smoother of include/ukf_batch.h ("fixed-interval smoothing"): the manifold
Rauch-Tung-Striebel backward pass over a window of filtered states, built from oracle.ukf_numpy (sigma_points, the process
models, mean_sigma_points, cov_sigma_points, cross_cov_sigma_points, cholesky_lower, apply_delta), the noise shaping of
pose_predict / orient_predict and the Jr^-1 of tests/bank_reference.py.  A helper, not collected;
tests/test_smoother_reference.py pins it.

Arrays are in WINDOW order (step 0 = the oldest): mu [steps, B, S], cov [steps, B, D, D], dt [steps - 1]; the optional input
rings in_a / in_b are [steps, B, 3] (step c's row serves the prediction c -> c + 1) or [B, 3] (latched)."""
import numpy as np

from oracle import ukf_numpy as on
from bank_reference import jr_inv, rot_offset


class Params:
    """what the engine holds at the time of the call"""

    def __init__(self, model, R, acc_cov=None, tau_g=1.0, tau_a=1.0, earth=(0.0, 0.0, 0.0), mean_tol=on.MEAN_TOL,
                 mean_max_it=on.MEAN_MAX_IT, min_dt=1e-9, max_dt=np.finfo(np.float64).max):
        self.model = model                      # "pose" / "orient"
        self.man = on.POSE if model == "pose" else on.ORIENT
        self.R = np.asarray(R, dtype=np.float64)  # [D, D] or [B, D, D]
        self.acc_cov = np.eye(3) if acc_cov is None else np.asarray(acc_cov, dtype=np.float64)
        self.tau_g, self.tau_a, self.earth = tau_g, tau_a, np.asarray(earth, dtype=np.float64)
        self.mean_tol, self.mean_max_it, self.min_dt, self.max_dt = mean_tol, mean_max_it, min_dt, max_dt


def _process_and_noise(p, mu, dt, in_a, in_b):
    """-> (g, R [B, D, D]): the process model of one prediction and its shaped noise, as pose_predict / orient_predict"""
    B, D = mu.shape[0], p.man.D
    Rn = np.broadcast_to(p.R, (B, D, D))
    d = np.full(B, float(dt))
    if p.model == "pose":
        use_acc = np.zeros(B, bool) if in_a is None else np.all(np.isfinite(in_a), axis=-1)
        rot = on.quat_to_matrix(mu[:, 3:7])
        Rcv = Rn.copy()
        Rcv[:, 0:3, 0:3] = on._rotate_block(rot, Rn, 0)
        Rcv[:, 3:6, 3:6] = on._rotate_block(rot, Rn, 3)
        Rcv = d[:, None, None] * Rcv
        Racc = Rn.copy()
        Racc[:, 6:9, 6:9] = 2.0 * p.acc_cov            # PoseUKF.cpp:190-191: raw noise, not scaled by dt
        R = np.where(use_acc[:, None, None], Racc, Rcv)
        a = np.where(use_acc[:, None], np.zeros((B, 3)) if in_a is None else in_a, 0.0)

        def g(X):
            return on.pose_process(X, a[:, None, :], d[:, None])   # a = 0: processModel (constant velocity)
        return g, R
    rot = on.quat_to_matrix(mu[:, 0:4])
    R = Rn.copy()
    R[:, 0:3, 0:3] = on._rotate_block(rot, Rn, 0)
    R[:, 3:6, 3:6] = on._rotate_block(rot, Rn, 3)
    R = (d * d)[:, None, None] * R

    def g(X):
        return on.orient_process(X, in_a[:, None, :], in_b[:, None, :], p.tau_g, p.tau_a, p.earth, d[:, None])
    return g, R


def backward_step(p, mu, cov, mu_s, cov_s, dt, in_a=None, in_b=None, transport=True):
    """One step of the recursion: (mu, cov) filtered at c, (mu_s, cov_s) smoothed at c + 1 -> smoothed at c and status [B]"""
    man = p.man
    B, D, ro = mu.shape[0], man.D, rot_offset(man)
    gate = on.gate_dt(np.full(B, float(dt)), p.min_dt, p.max_dt)
    if gate.any():   # one dt for the batch: gated for every filter
        return mu_s.copy(), cov_s.copy(), gate
    g, R = _process_and_noise(p, mu, dt, in_a, in_b)
    with np.errstate(all="ignore"):
        X, ok = on.sigma_points(man, mu, cov)
        Y = g(X)
        m_pred, conv = on.mean_sigma_points(man, Y, p.mean_tol, p.mean_max_it)
        Cp = on.cov_sigma_points(man, m_pred, Y) + R
        C = on.cross_cov_sigma_points(man, man, mu, m_pred, X, Y)
        _, ok_p = on.cholesky_lower(Cp)
        good = ok & ok_p
        Cp_s = np.where(good[:, None, None], Cp, np.eye(D)[None])
        G = np.swapaxes(np.linalg.solve(Cp_s, np.swapaxes(C, 1, 2)), 1, 2)
        e = man.boxminus(mu_s, m_pred)
        J = np.broadcast_to(np.eye(D), (B, D, D)).copy()
        if transport:
            J[:, ro:ro + 3, ro:ro + 3] = jr_inv(e[:, ro:ro + 3])
        St = J @ cov_s @ np.swapaxes(J, 1, 2)
        Sig = cov + G @ (St - Cp) @ np.swapaxes(G, 1, 2)
        Sig = np.tril(Sig) + np.swapaxes(np.tril(Sig, -1), 1, 2)   # the lower triangle is what is computed
        Sig_s = np.where(good[:, None, None] & np.isfinite(Sig).all(axis=(1, 2))[:, None, None], Sig, np.eye(D)[None])
        m, Cn, ok_c = on.apply_delta(man, mu, Sig_s, np.einsum("bij,bj->bi", G, e))
    good = good & ok_c & np.isfinite(Sig).all(axis=(1, 2))
    st = np.where(good, 0, on.ST_ERR_CHOLESKY) | np.where(conv | ~ok, 0, on.ST_WARN_MEAN_NOCONV)
    return np.where(good[:, None], m, mu), np.where(good[:, None, None], Cn, cov), st.astype(np.uint32)


def smooth(p, mu, cov, dt, in_a=None, in_b=None, initialised=None, transport=True):
    """-> (mu_s [steps, B, S], cov_s [steps, B, D, D], status [B], status_steps [steps - 1, B]).  Uninitialised filters keep
    NaN in the outputs (nothing is written for them) and report UNINITIALISED."""
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    steps, B = mu.shape[0], mu.shape[1]
    dt = np.asarray(dt, dtype=np.float64).reshape(steps - 1)
    mu_s, cov_s = mu.copy(), cov.copy()
    sts = np.zeros((steps - 1, B), dtype=np.uint32)
    ring = lambda x, c: None if x is None else (x[c] if np.ndim(x) == 3 else x)
    for c in range(steps - 2, -1, -1):
        mu_s[c], cov_s[c], sts[c] = backward_step(p, mu[c], cov[c], mu_s[c + 1], cov_s[c + 1], dt[c], ring(in_a, c), ring(in_b, c),
                                                  transport)
    status = np.bitwise_or.reduce(sts, axis=0)
    if initialised is not None:
        dead = ~np.asarray(initialised, dtype=bool)
        mu_s[:, dead], cov_s[:, dead] = np.nan, np.nan
        status = np.where(dead, on.ST_UNINITIALISED, status).astype(np.uint32)
    return mu_s, cov_s, status, sts


def window_order(ring, first_slot, steps):
    """steps consecutive slots of a ring [slots, ...], oldest first"""
    slots = ring.shape[0]
    return ring[[(first_slot + c) % slots for c in range(steps)]]
