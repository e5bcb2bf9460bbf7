"""The sampled update (tests/sampled_reference.update_sampled) with a dtype per stage, assembled from what tests/feature_f32.py
offers (update, vect, STATE, PRECISIONS): with every stage float32 it is the `d_32` of tests/feature_scaled_parity.py for a
plain fp32 engine, the drift a correct fp32 evaluation of the same algorithm shows on the same batch.  A helper, not collected.

The samples are the caller's, as stored.  As the kernel does (and as feature_f32.sensor_meas evaluates the sensor models in
float64 in every mode), the differences Z_i - Z_0 and z - Z_0 are formed in float64 first; the stages work on those differences
and z-bar gets Z_0 back in float64 before it is rounded to the storage type."""
import numpy as np

import feature_f32 as ff

F64 = np.float64


def update_sampled(model, mu, cov, Z, z, Q, keep=None, prec="f32"):
    """-> dict(mu, cov, z_pred [B, m], S [B, m, m], innov [B, m]); the state of `keep` rows (gated, failed) is unchanged"""
    P, man = ff.PRECISIONS[prec], ff.STATE[model]
    B, m = mu.shape[0], Z.shape[2]
    Q = np.broadcast_to(np.asarray(Q, dtype=F64), (B, m, m))
    keep = np.zeros(B, bool) if keep is None else np.asarray(keep, dtype=bool)
    z0 = np.asarray(Z[:, 0], dtype=F64)
    Zr = np.asarray(Z, dtype=F64) - z0[:, None, :]
    zr = np.asarray(z, dtype=F64) - z0
    parts = [Zr[:, 0], Zr[:, 1::2], Zr[:, 2::2]]   # feature_f32.statistics asks for h(X0), h(Xp), h(Xm) in this order

    def hh(X):
        return parts.pop(0).astype(X.dtype)
    r = ff.update(man, ff.vect(m), mu.astype(P.ts), cov.astype(P.ts), zr.astype(P.tm), hh, Q, P)
    assert not parts
    o = dict(mu=np.array(mu, dtype=F64), cov=np.array(cov, dtype=F64))
    go = ~keep
    o["mu"][go], o["cov"][go] = r["mu"][go], r["cov"][go]
    o["z_pred"] = (z0 + r["z_pred"]).astype(P.ts).astype(F64)
    o["S"], o["innov"] = r["S"], r["innov"]
    return o
