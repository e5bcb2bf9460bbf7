"""What the NumPy float64 references of the measurement features share, stated once: the scored update (ukfom's update through
oracle.ukf_numpy, the statistics it does not return, and the status rules of include/ukf_batch.h: which filters are scored,
which are committed, which status bits may coexist), the tail of the two updates that commit into the present through the
state history, the mean iteration with its trip counts, and the NaN-filled outputs.  Imported by tests/*_reference.py; a
helper, not collected; tests/test_update_reference.py pins it."""
import collections

import numpy as np

from oracle import ukf_numpy as on

Scored = collections.namedtuple("Scored", "Z mz S innov d2 logdet mu2 cov2 status commit scored ok")


def scored_update(man, manz, mu, cov, z, h, Q, tol, max_it, gate_chi2, *, extra_fail=None):
    """One update of the rows given: mu [B, S], cov [B, D, D], z [B, S_z], h: X [B, 2 D + 1, S] -> Z [B, 2 D + 1, S_z], Q
    [B, D_z, D_z] or a function of z-bar that returns it (a noise stated in z-bar's tangent frame), extra_fail [B]: rows that fail
    as if S had (ERR_CHOLESKY, nothing scored).  -> Scored: the sigma points' images Z, z-bar mz, S, the innovation, d^2 and
    log det S (of the identity where S failed), the state mu2, cov2 of on.ukf_update, status, and the masks commit (mu2, cov2
    are the new state), scored (mz ... logdet are results) and ok (Sigma's verdict).
    The status rules: ERR_CHOLESKY is or-ed in where Sigma, S or extra_fail failed; REJECTED_GATE is cleared where ERR_CHOLESKY
    is set.  A row is scored unless ERR_CHOLESKY, committed unless ERR_CHOLESKY or REJECTED_GATE."""
    # the statistics of the update, from the oracle's own pieces in the oracle's own order
    X, ok = on.sigma_points(man, mu, cov)
    Z = h(X)
    mz, _ = on.mean_sigma_points(manz, Z, tol, max_it)
    QQ = Q(mz) if callable(Q) else Q
    S = on.cov_sigma_points(manz, mz, Z) + QQ
    _, ok_s = on.cholesky_lower(S)
    ok_s &= ok if extra_fail is None else ok & ~extra_fail
    eye = np.eye(manz.D)
    S_safe = np.where(ok_s[:, None, None], S, eye)
    innov = manz.boxminus(z, mz)
    d2 = np.einsum("bi,bij,bj->b", innov, np.linalg.inv(S_safe), innov)
    logdet = np.linalg.slogdet(S_safe)[1]
    # (a filter whose Sigma or S is not positive definite gets the identity: its result is discarded below)
    m2, C2, s = on.ukf_update(man, manz, mu, np.where(ok[:, None, None], cov, np.eye(man.D)), z, h,
                              np.where(ok_s[:, None, None], QQ, eye), tol, max_it, gate_chi2)
    s = np.where(ok_s, s, s | on.ST_ERR_CHOLESKY).astype(np.uint32)
    s = np.where((s & on.ST_ERR_CHOLESKY) != 0, s & ~np.uint32(on.ST_REJECTED_GATE), s).astype(np.uint32)
    commit = (s & (on.ST_ERR_CHOLESKY | on.ST_REJECTED_GATE)) == 0
    scored = (s & on.ST_ERR_CHOLESKY) == 0
    return Scored(Z, mz, S, innov, d2, logdet, m2, C2, s, commit, scored, ok)


def commit_through_history(o, st, i, okc, ok2, accept, noconv, mz, S, nu, maha, loglik, si, ti, m2, C2):
    """The tail of an update that commits into the present (delayed_reference, relative_reference), for the rows i of one
    model: okc [k] every factorisation before the commit, ok2 the commit's own, accept the gate, noconv the capped means of
    rows whose mean was taken; mz, S, nu at the stored entries si and tangent entries ti of the padded outputs.  Writes the
    status bits into st[i] and the scores and the committed state into o."""
    okc = okc & (ok2 | ~accept)
    commit = okc & accept
    st[i] |= np.where(okc, 0, on.ST_ERR_CHOLESKY).astype(np.uint32)
    st[i] |= np.where(noconv, on.ST_WARN_MEAN_NOCONV, 0).astype(np.uint32)
    st[i] |= np.where(okc & ~accept, on.ST_REJECTED_GATE, 0).astype(np.uint32)
    s_ = i[okc]
    zp, Sp, nup = (np.zeros((len(i),) + o[k].shape[1:]) for k in ("z_pred", "S", "innov"))
    zp[:, si], nup[:, ti] = mz, nu
    Sp[:, ti[:, None], ti[None, :]] = S
    o["z_pred"][s_], o["S"][s_], o["innov"][s_] = zp[okc], Sp[okc], nup[okc]
    o["maha"][s_] = maha[okc]
    o["loglik"][s_] = loglik[okc]
    c_ = i[commit]
    o["mu"][c_], o["cov"][c_] = m2[commit], C2[commit]
    o["mu_out"][c_], o["cov_out"][c_] = m2[commit], C2[commit]
    o["committed"][c_] = True


def mean_iteration(man, X, tol=on.MEAN_TOL, max_it=on.MEAN_MAX_IT):
    """the iteration of on.mean_sigma_points once more, for what it does not return -> (trips [B]: steps whose norm exceeded
    tol (its `it`), norms [B, trips.max() + 1]: the norm of every step a filter made, NaN beyond its last)"""
    B, N, _ = X.shape
    ref = X[:, 0].copy()
    active, it, norms = np.ones(B, bool), np.zeros(B, np.int64), []
    while active.any():
        d = man.boxminus(X, ref[:, None, :])
        md = np.zeros((B, man.D))
        for i in range(N):
            md = md + d[:, i]
        md = md / float(N)
        nrm = np.sqrt(np.sum(md * md, axis=-1))
        norms.append(np.where(active, nrm, np.nan))
        ref = np.where(active[:, None], man.boxplus(ref, md), ref)
        big = nrm > tol
        it = np.where(active & big, it + 1, it)
        active = active & big & (it < max_it)
    return it, np.stack(norms, axis=1)


def nan_outputs(mu, cov, nz, m):
    """the outputs of a call before any filter is looked at: the state as it is, NaN scores (z_pred [B, nz], S [B, m, m],
    innov [B, m]), status 0"""
    B = mu.shape[0]
    return {"mu": mu.copy(), "cov": cov.copy(), "z_pred": np.full((B, nz), np.nan), "S": np.full((B, m, m), np.nan),
            "innov": np.full((B, m), np.nan), "maha": np.full(B, np.nan), "loglik": np.full(B, np.nan),
            "status": np.zeros(B, dtype=np.uint32)}
