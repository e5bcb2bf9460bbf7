"""The sensor-frame update with given weights with a dtype per stage: tests/pda_f32.py with the weights read instead of formed.
With every stage float32 it is what a correct all-float32 evaluation of ukfb_update_weighted_dev leaves, the `d_32` behind the
bounds of a plain fp32 engine in tests/test_gpu_weighted.py; with every stage float64 it is jpda_reference.update_weighted.  A
helper, not collected.

Status handling is the caller's, as in feature_f32: every row with a model of the engine is computed and must factorise;
`used` [K, B] is the set of weights the float64 reference used, and rows the reference does not commit are put back by `keep`."""
import numpy as np

import feature_f32 as ff
import pda_reference as pr
import sensor_meas_reference as smr
from feature_f32 import F64


def weighted(model, mu, cov, ids, zs, Q, mount, point, gyro, weight, used, keep=None, prec="f32"):
    """-> dict(mu, cov, z_pred [B, 3], S [B, 3, 3], innov [K, B, 3], maha, loglik, weight_used [K, B], beta0 [B], innov_comb
    [B, 3]) in float64 as stored in the engine's type; outputs of rows without a model of this engine are NaN and their state
    is unchanged"""
    P, man = ff.PRECISIONS[prec], ff.STATE[model]
    K, B = zs.shape[0], mu.shape[0]
    ids = np.broadcast_to(np.asarray(ids, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=F64), (B, 3, 3))
    mount = np.broadcast_to(np.asarray(mount, dtype=F64), (B, 7))
    point = np.broadcast_to(np.asarray(point, dtype=F64), (B, 3))
    gyro = np.zeros((B, 3)) if gyro is None else np.asarray(gyro, dtype=F64)
    keep = np.zeros(B, bool) if keep is None else np.asarray(keep, dtype=bool)
    nanf = lambda *s: np.full(s, np.nan)   # noqa: E731
    o = dict(mu=np.array(mu, dtype=F64), cov=np.array(cov, dtype=F64), z_pred=nanf(B, 3), S=nanf(B, 3, 3), innov=nanf(K, B, 3),
             maha=nanf(K, B), loglik=nanf(K, B), weight_used=nanf(K, B), beta0=nanf(B), innov_comb=nanf(B, 3))
    st = lambda x: x.astype(P.ts).astype(F64)   # noqa: E731
    own = smr.POSE_IDS if model == "pose" else smr.ORIENT_IDS
    for mid in np.unique(ids[np.isin(ids, own)]):
        mid = int(mid)
        m = smr.meas_dim(mid)
        idx = np.nonzero(ids == mid)[0]
        _, _, um, up = smr.used_inputs(mid)
        mt = np.where(um, mount[idx], smr.IDENTITY_MOUNT)[:, None, :]
        pt = np.where(up, point[idx], 0.0)[:, None, :]
        gy = gyro[idx][:, None, :]

        def hh(X):   # float64 in every mode: the kernel evaluates the sensor models in double
            one = X.ndim == 2
            return smr.h(mid, X.astype(F64), mt[:, 0] if one else mt, pt[:, 0] if one else pt, gy[:, 0] if one else gy).astype(X.dtype)
        manz = ff.vect(m)
        mu_i = mu[idx].astype(P.ts)
        s = ff.statistics(man, manz, mu_i, cov[idx].astype(P.ts), hh, Q[idx][:, :m, :m], P)
        nu = np.stack([ff.innovation(manz, zs[k][idx][:, :m].astype(P.ts), s["zbar"], P) for k in range(K)])
        Si = np.linalg.inv(s["S"])
        G = used[:, idx]
        d2 = np.einsum("kbi,bij,kbj->kb", nu, Si, nu)
        loglik = (-0.5 * (d2 + np.linalg.slogdet(s["S"])[1][None] + m * smr.LN_2PI)).astype(P.tl)
        wk = np.where(G, np.nan_to_num(weight[:, idx]), 0.0).astype(P.ts).astype(P.tl)
        total = wk.sum(axis=0, dtype=P.tl)
        c = np.maximum(P.tl(1), total)
        beta, beta0 = (wk / c[None]).astype(P.tl), (P.tl(1) - total / c).astype(P.tl)
        cov2, delta, nub = pr.combine_textbook(s["cov"], s["Cxz"] @ Si, s["S"], np.where(G[:, :, None], nu, 0), beta, beta0, P.tl)
        cov2 = 0.5 * (cov2 + np.swapaxes(cov2, 1, 2))
        go = ~keep[idx] & G.any(axis=0)
        cov2 = np.where(go[:, None, None], cov2, s["cov"])   # (a row that is not committed: anything that factorises)
        m2, C2 = ff.apply_delta(man, mu_i, cov2, np.where(go[:, None], delta, 0).astype(P.tl), P)
        o["mu"][idx[go]], o["cov"][idx[go]] = st(m2)[go], st(C2)[go]
        o["z_pred"][idx], o["S"][idx], o["innov"][:, idx], o["innov_comb"][idx] = 0.0, 0.0, 0.0, 0.0
        o["z_pred"][idx, :m], o["innov_comb"][idx, :m] = st(s["zbar"]), st(nub)
        o["innov"][:, idx, :m] = st(nu)
        o["S"][idx[:, None, None], np.arange(m)[None, :, None], np.arange(m)[None, None, :]] = st(s["S"])
        o["weight_used"][:, idx], o["beta0"][idx] = st(beta), st(beta0)
        o["maha"][:, idx], o["loglik"][:, idx] = st(d2), st(loglik)
    return o
