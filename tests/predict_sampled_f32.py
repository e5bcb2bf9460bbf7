"""The sampled prediction (tests/predict_sampled_reference.predict_sampled) with a dtype per stage, assembled from what
tests/feature_f32.py offers (manifold_mean, STATE, PRECISIONS): with every stage float32 it is the `d_32` of
tests/feature_scaled_parity.py for a plain fp32 engine, the drift a correct fp32 evaluation of the same algorithm shows on the
same batch.  A helper, not collected.

The propagated points are the caller's, as stored.  As the kernel does, the differences XX_i - XX_0 of the vector blocks are
formed in float64 first; the stages work on those differences (quaternion blocks as they are) and the vector blocks of the mean
get XX_0 back in float64 before they are rounded to the storage type."""
import numpy as np

import feature_f32 as ff

F64 = np.float64


def predict_sampled(model, mu, cov, XX, R, keep=None, prec="f32"):
    """-> dict(mu, cov); the state of `keep` rows (inactive, failed) is unchanged"""
    P, man = ff.PRECISIONS[prec], ff.STATE[model]
    B, D = mu.shape[0], man.D
    R = np.broadcast_to(np.asarray(R, dtype=F64), (B, D, D))
    R = np.where(np.tril(np.ones((D, D), bool)), R, np.swapaxes(R, 1, 2))
    keep = np.zeros(B, bool) if keep is None else np.asarray(keep, dtype=bool)
    XX = np.asarray(XX, dtype=F64)
    x0 = XX[:, 0].copy()
    rel = XX.copy()
    for kind, so, _, n in man.fields:
        if kind == "so3":
            x0[:, so:so + 4] = 0.0
        else:
            rel[:, :, so:so + n] = XX[:, :, so:so + n] - XX[:, 0:1, so:so + n]
    X0, Xp, Xm = rel[:, 0].astype(P.tc), rel[:, 1::2].astype(P.tm), rel[:, 2::2].astype(P.tm)
    mean = ff.manifold_mean(man, X0, Xp, Xm, P)
    mm = mean.astype(P.tm)[:, None, :]
    dp, dm = man.minus(Xp, mm).astype(P.tl), man.minus(Xm, mm).astype(P.tl)
    d0 = man.minus(X0.astype(P.tm), mm[:, 0]).astype(P.tl)
    C = 0.5 * (ff._outer_sum(dp, dp) + ff._outer_sum(dm, dm) + d0[:, :, None] * d0[:, None, :]) + R.astype(P.tl)
    o = dict(mu=np.array(mu, dtype=F64), cov=np.array(cov, dtype=F64))
    go = ~keep
    o["mu"][go] = (x0 + mean.astype(F64)).astype(P.ts).astype(F64)[go]
    o["cov"][go] = C.astype(P.ts).astype(F64)[go]
    return o
