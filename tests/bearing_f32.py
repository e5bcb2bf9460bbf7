"""The bearing update (tests/bearing_reference.update_bearing) with a dtype per stage, on tests/feature_f32.py's `update`: with
every stage float32 it is the `d_32` of tests/feature_scaled_parity.py for a plain fp32 engine, the drift a correct fp32
evaluation of the same algorithm shows on the same batch; with every stage float64 it is the reference.  A helper, not collected.

As the kernel does (and as feature_f32.sensor_meas evaluates the sensor models in float64 in every mode), h and the sphere's
exponential and logarithm are evaluated in float64 and handed back in the dtype of the stage that asked.  The update is the
2 x 2 basis form of the reference; feature_f32.update wants its noise up front, so the statistics run once for z-bar, whose
tangent basis gives Q2 = B^T Q B, and the update then runs with it (z-bar comes out the same: it does not depend on Q).  S and
nu are lifted to the ambient frame with B in float64 and rounded to the storage type once."""
import numpy as np

import bearing_reference as br
import feature_f32 as ff

F64 = np.float64


class S2:
    """the sphere in the interface of study_f32_mixed.Man / feature_f32.Fields (S, D, plus, minus)"""
    S, D = 3, 2

    def minus(self, x, y):
        t = np.result_type(x, y)
        x, y = np.broadcast_arrays(np.asarray(x, dtype=F64), np.asarray(y, dtype=F64))
        return np.einsum("...ij,...i->...j", br.basis_duff(y), br.s2_log(y, x)).astype(t)

    def plus(self, x, d):
        t = np.result_type(x, d)
        x = np.asarray(x, dtype=F64)
        return br.s2_exp(x, np.einsum("...ij,...j->...i", br.basis_duff(x), np.asarray(d, dtype=F64))).astype(t)


def update_bearing(model, mu, cov, ids, z, Q, mount, point, keep=None, prec="f32"):
    """-> dict(mu, cov, z_pred [B, 3], S [B, 3, 3], innov [B, 3]); outputs of rows without a model of this engine are NaN, their
    state and that of `keep` rows (gated, failed) is unchanged"""
    P, man, manz = ff.PRECISIONS[prec], ff.STATE[model], S2()
    B = mu.shape[0]
    ids = np.broadcast_to(np.asarray(ids, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=F64), (B, 3, 3))
    mount = np.broadcast_to(np.asarray(mount, dtype=F64), (B, 7))
    point = np.broadcast_to(np.asarray(point, dtype=F64), (B, 3))
    keep = np.zeros(B, bool) if keep is None else np.asarray(keep, dtype=bool)
    o = dict(mu=np.array(mu, dtype=F64), cov=np.array(cov, dtype=F64), z_pred=np.full((B, 3), np.nan), S=np.full((B, 3, 3), np.nan),
             innov=np.full((B, 3), np.nan))
    own = br.POSE_IDS if model == "pose" else br.ORIENT_IDS
    for mid in np.unique(ids[np.isin(ids, own)]):
        mid = int(mid)
        idx = np.nonzero(ids == mid)[0]
        mt = np.where(br.used_inputs(mid)[0], mount[idx], br.sr.IDENTITY_MOUNT)[:, None, :]
        pt = point[idx][:, None, :]
        Q3 = np.tril(Q[idx]) + np.swapaxes(np.tril(Q[idx], -1), 1, 2)

        def hh(X):
            one = X.ndim == 2
            return br.unit(br.direction(mid, X.astype(F64), mt[:, 0] if one else mt, pt[:, 0] if one else pt)).astype(X.dtype)
        m_, c_ = mu[idx].astype(P.ts), cov[idx].astype(P.ts)
        zbar = ff.statistics(man, manz, m_, c_, hh, np.zeros((idx.size, 2, 2)), P)["zbar"]
        Bz = br.basis_duff(zbar.astype(F64))
        Q2 = np.swapaxes(Bz, 1, 2) @ Q3 @ Bz
        zhat = br.unit(z[idx].astype(P.ts).astype(F64))
        r = ff.update(man, manz, m_, c_, zhat, hh, Q2, P)
        assert np.array_equal(r["z_pred"], zbar.astype(P.ts).astype(F64))
        go = ~keep[idx]
        o["mu"][idx[go]], o["cov"][idx[go]] = r["mu"][go], r["cov"][go]
        st = lambda x: x.astype(P.ts).astype(F64)   # noqa: E731
        o["z_pred"][idx] = r["z_pred"]
        o["S"][idx] = st(Bz @ r["S"] @ np.swapaxes(Bz, 1, 2))
        o["innov"][idx] = st(np.einsum("bij,bj->bi", Bz, r["innov"]))
    return o
