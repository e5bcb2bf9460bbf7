"""NumPy statement of the filter-bank definitions of include/ukf_batch.h ("filter banks") on oracle.ukf_numpy's compounds
(POSE / ORIENT: boxplus, boxminus).  A helper, not collected; tests/test_bank_reference.py pins it.

Arrays: mu [T, M, S], cov [T, M, D, D], w [T, M]; every function works on a batch of T tracks."""
import numpy as np

MEAN_TOL, MEAN_MAX_IT = 1e-6, 10000


def rot_offset(man):
    """tangent offset of the SO(3) component"""
    return [to for kind, _, to, _ in man.fields if kind == "so3"][0]


def hat(p):
    H = np.zeros(p.shape[:-1] + (3, 3))
    H[..., 0, 1], H[..., 0, 2] = -p[..., 2], p[..., 1]
    H[..., 1, 0], H[..., 1, 2] = p[..., 2], -p[..., 0]
    H[..., 2, 0], H[..., 2, 1] = -p[..., 1], p[..., 0]
    return H


def jr_inv(p):
    """Jr^-1(phi) = I + [phi]x / 2 + c(theta) [phi]x^2, c = (1 - (theta/2) cot(theta/2)) / theta^2 in the half-angle form
    (sin(theta/2) - (theta/2) cos(theta/2)) / (theta^2 sin(theta/2)): no cancellation towards theta = pi (c = 1/pi^2) and no
    zero denominator below the pole of Jr^-1 at 2 pi; 1/theta^2 - (1 + cos theta) / (2 theta sin theta) is 0/0 at pi"""
    th = np.sqrt(np.sum(p * p, axis=-1))
    small = th < 1e-2
    h = 0.5 * np.where(small, 1.0, th)
    c = np.where(small, 1.0 / 12.0 + th * th / 720.0, (np.sin(h) - h * np.cos(h)) / (4.0 * h * h * np.sin(h)))
    H = hat(p)
    return np.eye(3) + 0.5 * H + c[..., None, None] * (H @ H)


def mixture(man, mu, cov, w, tol=MEAN_TOL, max_it=MEAN_MAX_IT, transport=True):
    """Mixture moments of T tracks -> (mean [T, S], cov [T, D, D], converged [T]).  A hypothesis of weight exactly 0 is
    skipped (selected out), so that a NaN state of weight 0 never reaches the result.  transport=False leaves J_j out."""
    T, M, _ = mu.shape
    D, ro = man.D, rot_offset(man)
    tr = np.arange(T)
    used = w != 0.0
    ref = mu[tr, np.argmax(np.where(used, w, -1.0), axis=1)].copy()   # argmax: the first of equal weights
    active, it, conv = np.ones(T, bool), np.zeros(T, np.int64), np.ones(T, bool)
    while active.any():
        d = np.zeros((T, D))
        for j in range(M):
            with np.errstate(all="ignore"):
                dj = man.boxminus(mu[:, j], ref)
            d = d + np.where(used[:, j, None], w[:, j, None] * dj, 0.0)
        norm = np.sqrt(np.sum(d * d, axis=-1))
        ref = np.where(active[:, None], man.boxplus(ref, d), ref)
        big = norm > tol
        it = np.where(active & big, it + 1, it)
        conv &= ~(active & big & (it >= max_it))
        active = active & big & (it < max_it)
    C = np.zeros((T, D, D))
    for j in range(M):
        with np.errstate(all="ignore"):
            dj = man.boxminus(mu[:, j], ref)
            J = np.broadcast_to(np.eye(D), (T, D, D)).copy()
            if transport:
                J[:, ro:ro + 3, ro:ro + 3] = jr_inv(dj[:, ro:ro + 3])
            term = w[:, j, None, None] * (J @ cov[:, j] @ np.swapaxes(J, 1, 2) + dj[:, :, None] * dj[:, None, :])
        C = C + np.where(used[:, j, None, None], term, 0.0)
    return ref, C, conv


def mixing_weights(w, P):
    """c [T, M] (c_i = sum_j P[j][i] w_j) and wji [T, M(i), M(j)] = P[j][i] w_j / c_i (row i one-hot on i where c_i = 0)"""
    M = w.shape[1]
    c = w @ P
    with np.errstate(all="ignore"):
        wji = (P.T[None, :, :] * w[:, None, :]) / c[:, :, None]
    wji = np.where((c > 0)[:, :, None], wji, np.eye(M)[None])
    return c, wji


def mix(man, mu, cov, w, P, **kw):
    """IMM interaction -> (mu' [T, M, S], cov' [T, M, D, D], w_pred [T, M], converged [T]); c_i = 0 keeps hypothesis i"""
    c, wji = mixing_weights(w, P)
    mu_o, cov_o, conv = mu.copy(), cov.copy(), np.ones(mu.shape[0], bool)
    for i in range(mu.shape[1]):
        m, C, cv = mixture(man, mu, cov, wji[:, i], **kw)
        go = c[:, i] > 0
        mu_o[go, i], cov_o[go, i] = m[go], C[go]
        conv &= cv | ~go
    return mu_o, cov_o, c, conv


def weights(logw_in, loglik, M=None):
    """-> (logw_out [T, M], w_out [T, M], all_dead [T]).  NaN loglik: dead; all dead: logw_in normalised on its own."""
    if logw_in is None:
        logw_in = np.zeros_like(loglik)
    a = logw_in if loglik is None else logw_in + loglik
    a = np.where(np.isnan(a), -np.inf, a)
    dead = ~np.isfinite(a.max(axis=1))
    a = np.where(dead[:, None], np.where(np.isnan(logw_in), -np.inf, logw_in), a)
    a = np.where(~np.isfinite(a.max(axis=1))[:, None], 0.0, a)
    with np.errstate(all="ignore"):
        d = a - a.max(axis=1, keepdims=True)
        e = np.exp(d)
        s = e.sum(axis=1, keepdims=True)
        return d - np.log(s), e / s, dead


def make_tracks(spe, onp, model, T, M, spread=0.33, seed=7):
    """T tracks of M hypotheses: a synthetic initial state and M tangent steps of about its own sigma, the rotation part spread
    up to `spread` rad (the prototype's construction)."""
    man = onp.POSE if model == "pose" else onp.ORIENT
    mu0, cov0 = (spe.synth.pose_initial if model == "pose" else spe.synth.orient_initial)(T * M)
    rng = np.random.default_rng(seed)
    base = mu0[::M]
    sig = np.sqrt(np.einsum("tii->ti", cov0[::M]))
    step = rng.standard_normal((T, M, man.D)) * sig[:, None, :]
    ro = rot_offset(man)
    step[:, :, ro:ro + 3] = rng.uniform(-1, 1, (T, M, 3)) * spread / np.sqrt(3.0)
    mu = man.boxplus(base[:, None, :], step)
    cov = cov0.reshape(T, M, man.D, man.D).copy()
    w = rng.uniform(0.05, 1.0, (T, M))
    w /= w.sum(axis=1, keepdims=True)
    return man, mu, cov, w


def transition(M, seed=11):
    rng = np.random.default_rng(seed)
    P = 0.6 * np.eye(M) + 0.4 * rng.uniform(0.1, 1.0, (M, M))
    return P / P.sum(axis=1, keepdims=True)
