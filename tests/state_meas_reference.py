"""NumPy float64 statement of the joint state-block measurement of include/ukf_batch.h ("joint state-block measurements"):
the scored update of tests/update_reference.py (oracle.ukf_numpy.ukf_update, what it does not return, the status rules of the
header) with the measurement manifold the compound of the selected state blocks and h their selection.  A helper, not
collected; tests/test_state_meas_reference.py pins it."""
import numpy as np

from oracle import ukf_numpy as on
from update_reference import scored_update

LN_2PI = float(np.log(2.0 * np.pi))


def sub_manifold(man, mask):
    """-> (the compound of the blocks `mask` selects, in state order; their stored indices; their tangent indices)"""
    fields, stored, tangent, so, to = [], [], [], 0, 0
    for b, (kind, s0, t0, n) in enumerate(man.fields):
        if (int(mask) >> b) & 1:
            ns, nt = (4, 3) if kind == "so3" else (n, n)
            fields.append((kind, so, to, n))
            stored += list(range(s0, s0 + ns))
            tangent += list(range(t0, t0 + nt))
            so, to = so + ns, to + nt
    return on._Compound(fields), np.array(stored, dtype=np.int64), np.array(tangent, dtype=np.int64)


def mask_valid(man, masks):
    masks = np.asarray(masks, dtype=np.int64)
    return (masks > 0) & ((masks >> len(man.fields)) == 0)


def update_state(man, mu, cov, masks, z, Qz, a=1.0, b=1.0, gate_chi2=-1.0, initialised=None, tol=on.MEAN_TOL,
                 max_it=on.MEAN_MAX_IT):
    """mu [B, S], cov [B, D, D], masks an int or [B], z [B, S], Qz [B, D, D] -> (mu, cov, maha [B], loglik [B], status [B]).
    Filters are grouped by mask; every group is one scored update on a * cov and b * Qz[sel][sel]."""
    B = mu.shape[0]
    masks = np.broadcast_to(np.asarray(masks, dtype=np.int64), (B,))
    init = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    mu_o, cov_o = mu.copy(), cov.copy()
    maha, ll = np.full(B, np.nan), np.full(B, np.nan)
    st = np.zeros(B, dtype=np.uint32)
    valid = mask_valid(man, masks)
    st[~init] = on.ST_UNINITIALISED
    st[init & ~valid] = on.ST_INACTIVE
    for m in np.unique(masks[init & valid]):
        idx = np.nonzero(init & valid & (masks == m))[0]
        manz, si, ti = sub_manifold(man, int(m))
        zz, QQ = z[idx][:, si], Qz[idx][:, ti[:, None], ti[None, :]]
        fin = np.isfinite(zz).all(axis=1) & np.isfinite(QQ).all(axis=(1, 2))
        st[idx[~fin]] = on.ST_ERR_NONFINITE_MEAS
        idx, zz, QQ = idx[fin], zz[fin], b * QQ[fin]
        if idx.size == 0:
            continue
        u = scored_update(man, manz, mu[idx], a * cov[idx], zz, lambda X: X[..., si], QQ, tol, max_it, gate_chi2)
        mu_o[idx[u.commit]], cov_o[idx[u.commit]] = u.mu2[u.commit], u.cov2[u.commit]
        maha[idx] = np.where(u.scored, u.d2, np.nan)
        ll[idx] = np.where(u.scored, -0.5 * (u.d2 + u.logdet + manz.D * LN_2PI), np.nan)
        st[idx] = u.status
    return mu_o, cov_o, maha, ll, st


def full_mask(model):
    return 15 if model == "pose" else 31


def make_inputs(man, mu, cov, dtype, seed=11):
    """the joint measurement the tests update with: z = mu (+) L xi, Qz = Sigma + (L A)(L A)^T, as the engine stores them"""
    n = mu.shape[0]
    rng = np.random.default_rng(seed)
    L = np.linalg.cholesky(cov)
    z = man.boxplus(mu, np.einsum("bij,bj->bi", L, rng.standard_normal((n, man.D))))
    LA = L @ (0.3 * rng.standard_normal((n, man.D, man.D)))
    Qz = cov + LA @ np.swapaxes(LA, 1, 2)
    Qz = 0.5 * (Qz + np.swapaxes(Qz, 1, 2))
    return z.astype(dtype).astype(np.float64), Qz.astype(dtype).astype(np.float64)


def cycling_masks(model, n):
    """every mask of the model, 0 included, so that four wave-mates always differ"""
    return (np.arange(n) % (full_mask(model) + 1)).astype(np.int32)
