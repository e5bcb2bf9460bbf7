"""Scale-aware parity for the five feature kernels (innovation statistics, filter banks, the smoother, state-block and
sensor-frame measurements): tests/scaled_parity.py pointed at their outputs.  A helper, not collected;
tests/test_feature_scaled_reference.py pins it, the five tests/test_gpu_*.py feature files and tools/scaled_parity_report.py
call it.

STATE outputs (mu, C) -- an updated state, every step of a smoothed window, every mixed hypothesis, the combined moments -- are
judged exactly as scaled_parity.distances does: whitened by the reference's own s_i = sqrt(C_ref[i, i]), the oracle's boxminus,
the maximum over all filters (steps and hypotheses flattened into the batch) per mean block and per pair of covariance blocks.

MEASUREMENT-SPACE outputs z-bar, S, nu are whitened by s^z_i = sqrt(S_ref[i, i]):

    |dS|_ij / (s^z_i s^z_j)      |d nu_i| / s^z_i      |(z-bar (-) z-bar_ref)_i| / s^z_i   ((-) of the measurement manifold)

and reduced to the maximum over filters, entries and candidates per output.  d^2, the log-likelihood and the bank weights are
dimensionless (or offset by logdet) and stay on the bound their files already hold them to.

Bounds, u = 2^-24, none of them from GPU output:

    fp64 engines   1e-9 (scaled_parity.TOL_F64)
    wide fp32      2 u v + 1e-9 against the float64 reference on the inputs as stored: scaled_parity.bound_wide with c = 1.  Each
                   of the five kernels narrows a stored output exactly once (the TS(...) at its stores; ukf_smooth.hpp keeps the
                   chain CSM / CSP in T and narrows each step's record once, the chain itself never).  State outputs: v =
                   mean_scale for the mean, 1 for the covariance.  Measurement space, entry by entry: v = 1 for S,
                   |nu_i| / s^z_i for nu, max(1, |z-bar_i|) / s^z_i for z-bar (2 / s^z_i for a rotation coordinate).
    plain fp32     max(M_FEAT d_32, 20 u v): d_32 is the same block's distance between the all-float32 and the all-float64
                   evaluation of tests/feature_f32.py on the same batch; the floor is scaled_parity.FLOOR_ULP.

M_FEAT = max(scaled_parity.M, 2 x the largest per-block ratio between two independent correct fp32 evaluations of a feature):
the C++ float oracle's update computes the same thing as a state-block measurement of one Euclidean block and as a
sensor-frame measurement with r = 0 and qs the identity.  tests/test_feature_scaled_reference.py recomputes it
(profiles/feature_scaled_parity.txt); it is never taken from a GPU result."""
import numpy as np

import scaled_parity as sp
from scaled_parity import U, TOL_F64, FLOOR_ULP

# profiles/feature_scaled_parity.txt ("M_feat ="): the largest ratio found there is below scaled_parity.M / 2
M_FEAT = 7.0

MODE = {"f64": "f64", "f32": "f32", "f32w": "wide", "wide": "wide"}
REPORT = []   # (name, mode, kind, rows of (label, distance, bound)) of every comparison made, for tools/scaled_parity_report.py


def _flat(model, mu, C):
    S, D = (13, 12) if model == "pose" else (14, 13)
    return np.asarray(mu, dtype=np.float64).reshape(-1, S), np.asarray(C, dtype=np.float64).reshape(-1, D, D)


def _rows(dist, bound):
    names = sp.block_names(dist.model)
    B = len(names)
    out = [(f"mean[{a}]", dist.mean[i], bound.mean[i]) for i, a in enumerate(names)]
    out += [(f"cov[{names[i]},{names[j]}]", dist.cov[i, j], bound.cov[i, j]) for i in range(B) for j in range(i, B)]
    return out


def _line(name, mode, kind, rows):
    """the SCALED line: the largest ratio of distance to bound and the block it belongs to"""
    worst = max(rows, key=lambda r: np.inf if np.isnan(r[1]) else r[1] / r[2])
    ratio = worst[1] / worst[2]
    REPORT.append((name, mode, kind, rows))
    print(f"SCALED {name} mode={mode} {kind} worst={ratio:.3e} of its bound at {worst[0]} (distance {worst[1]:.3e}, bound {worst[2]:.3e})")
    return ratio, worst[0]


def state_bound(model, mode, mu_ref, C_ref, d_32=None, commits=1):
    if mode == "f64":
        return sp.bound_f64(model)
    if mode == "wide":
        return sp.bound_wide(model, mu_ref, C_ref, commits)
    return sp.bound_f32(model, mu_ref, C_ref, d_32, margin=M_FEAT)


def judge_state(name, model, mode, mu, C, mu_ref, C_ref, f32=None, rows=None):
    """The scaled check of state outputs.  mu [..., S], C [..., D, D]: leading axes (steps, hypotheses, filters) are flattened,
    `rows` selects among the flattened rows (default: all).  mode: "f64" / "f32" / "wide" (or a test file's "f32w").
    f32: for a plain fp32 engine, a callable -> ((mu32, C32), (mu64, C64)), the two evaluations of tests/feature_f32.py on the
    same batch and rows' shape as mu / C; None leaves the plain-fp32 check out (no bound is known) and says so in the line."""
    mode = MODE[mode]
    mu, C = _flat(model, mu, C)
    mu_ref, C_ref = _flat(model, mu_ref, C_ref)
    idx = np.arange(mu.shape[0]) if rows is None else np.arange(mu.shape[0])[rows]
    d = sp.distances(model, mu[idx], C[idx], mu_ref[idx], C_ref[idx], idx)
    d_32 = None
    if mode == "f32":
        if f32 is None:
            print(f"SCALED {name} mode=f32 state: no fp32 evaluation of this call, scaled check left out")
            return None
        (m32, c32), (m64, c64) = f32()
        m32, c32 = _flat(model, m32, c32)
        m64, c64 = _flat(model, m64, c64)
        d_32 = sp.distances(model, m32[idx], c32[idx], m64[idx], c64[idx], idx)
    b = state_bound(model, mode, mu_ref[idx], C_ref[idx], d_32)
    _line(name, mode, "state", _rows(d, b))
    sp.check(d, b, f"{name} [{mode} {model}]")
    return d, b


# ------------------------------------------------------------------------------------------------ measurement space
def _so3_minus(q, q_ref):
    from oracle import ukf_numpy as on
    return on.so3_boxminus(np.asarray(q, dtype=np.float64), np.asarray(q_ref, dtype=np.float64))


def meas_distances(zbar, S, nu, zbar_ref, S_ref, nu_ref, so3=False):
    """-> {"S": [n, m, m], "nu": [..., n, m], "z_pred": [n, m]} whitened entry by entry, and s^z [n, m]"""
    S, S_ref = np.asarray(S, dtype=np.float64), np.asarray(S_ref, dtype=np.float64)
    s = np.sqrt(np.einsum("nii->ni", S_ref))
    dz = _so3_minus(zbar, zbar_ref) if so3 else np.asarray(zbar, dtype=np.float64) - np.asarray(zbar_ref, dtype=np.float64)
    return {"S": np.abs(S - S_ref) / (s[:, :, None] * s[:, None, :]),
            "nu": np.abs(np.asarray(nu, dtype=np.float64) - np.asarray(nu_ref, dtype=np.float64)) / s,
            "z_pred": np.abs(dz) / s}, s


def meas_scale(zbar_ref, S_ref, nu_ref, so3=False):
    """v entry by entry: 1 for S, |nu_i| / s^z_i, max(1, |z-bar_i|) / s^z_i (2 / s^z_i for a rotation coordinate)"""
    s = np.sqrt(np.einsum("nii->ni", np.asarray(S_ref, dtype=np.float64)))
    mz = np.full(s.shape, 2.0) if so3 else np.maximum(1.0, np.abs(np.asarray(zbar_ref, dtype=np.float64)))
    return {"S": np.ones(np.shape(S_ref)), "nu": np.abs(np.asarray(nu_ref, dtype=np.float64)) / s, "z_pred": mz / s}


def meas_bound(mode, v, d_32=None):
    """entry-by-entry bounds of the three outputs; d_32: {"S", "nu", "z_pred"} -> the fp32 evaluation's maximum of that output"""
    if mode == "f64":
        return {k: np.full(np.shape(x), TOL_F64) for k, x in v.items()}
    if mode == "wide":
        return {k: 2.0 * U * x + 1e-9 for k, x in v.items()}
    return {k: np.maximum(M_FEAT * d_32[k], FLOOR_ULP * U * x) for k, x in v.items()}


def judge_meas(name, mode, zbar, S, nu, zbar_ref, S_ref, nu_ref, so3=False, f32=None):
    """The scaled check of z-bar [n, m] (quaternions [n, 4] when so3), S [n, m, m] and nu [n, m] or [K, n, m] of the scored
    filters.  f32: a callable -> ((zbar32, S32, nu32), (zbar64, S64, nu64)) for a plain fp32 engine."""
    mode = MODE[mode]
    if np.shape(S)[0] == 0:
        return None
    d, _ = meas_distances(zbar, S, nu, zbar_ref, S_ref, nu_ref, so3)
    v = meas_scale(zbar_ref, S_ref, nu_ref, so3)
    d_32 = None
    if mode == "f32":
        if f32 is None:
            print(f"SCALED {name} mode=f32 measurement: no fp32 evaluation of this call, scaled check left out")
            return None
        a, b = f32()
        d_32 = {k: float(x.max()) for k, x in meas_distances(a[0], a[1], a[2], b[0], b[1], b[2], so3)[0].items()}
    bound = meas_bound(mode, v, d_32)
    rows = []
    for k in ("z_pred", "S", "nu"):
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(d[k] == 0.0, 0.0, d[k] / bound[k])   # a NaN distance stays NaN and fails below
        at = np.unravel_index(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
        rows.append((k, float(d[k][at]), float(bound[k][at])))
    _line(name, mode, "measurement", rows)
    bad = [(k, dist, bnd) for k, dist, bnd in rows if not dist <= bnd]
    assert not bad, f"{name} [{mode}]: " + "; ".join(f"output {k}: {x:.3e} > bound {t:.3e}" for k, x, t in bad)
    return rows


# ------------------------------------------------------------------------------------------------ CPU: the GPU files' input families
ACC_COV = 0.01 * np.eye(3)


def cycled_state(spe, model, n, prec=0, cycles=2):
    """synth.pose_initial / orient_initial after `cycles` real cycles by the C++ oracle (prec 0: fp64, 1: the float oracle with
    the state rounded to float at every cycle): what cycled_engine of tests/engine_support.py
    downloads from an engine, without one"""
    from oracle import capi, ukf_numpy as on
    sy = spe.synth
    r = sp.f32r if prec else (lambda x: np.asarray(x, dtype=np.float64))
    mu, cov = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
    mu, cov = r(mu), r(cov)
    for c in range(cycles):
        if model == "pose":
            acc, z, Q = sy.pose_cycle_inputs(n, c, mu[:, :3])
            mu, cov, s1 = capi.pose_predict(mu, cov, r(sy.pose_default_process_noise()), r(acc), r(ACC_COV), 0.01, prec=prec)
            mu, cov, s2 = capi.pose_update(mu, cov, spe.MEAS_POS3, r(z), r(Q), prec=prec)
        else:
            gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu[:, 0:4])
            mu, cov, s1 = capi.orient_predict(mu, cov, r(sy.orient_process_noise()), r(acc), r(gyro), sy.ORIENT_TAU, sy.ORIENT_TAU,
                                              on.earth_rotation(sy.ORIENT_LATITUDE), 0.01, prec=prec)
            mu, cov, s2 = capi.orient_update(mu, cov, r(z), r(Q), prec=prec)
        assert (s1 == 0).all() and (s2 == 0).all()
        mu, cov = r(mu), r(cov)
    return mu, cov


def recorded_window(spe, model, n, steps, prec=0, per_filter_noise=False):
    """the history of tests/test_gpu_smooth.record by the C++ oracle -> (params of smoother_reference, mu [steps, n, S],
    cov [steps, n, D, D], dt [steps - 1], in_a [steps, n, 3], in_b [steps, n, 3])"""
    from oracle import capi, ukf_numpy as on
    import smoother_reference as smr
    sy = spe.synth
    r = sp.f32r if prec else (lambda x: np.asarray(x, dtype=np.float64))
    mu, cov = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
    mu, cov = r(mu), r(cov)
    dt = np.array([0.01 * (1.0 + 0.1 * c) for c in range(steps - 1)])
    R = r(sy.pose_default_process_noise() if model == "pose" else sy.orient_process_noise())
    if per_filter_noise:   # every filter its own matrix, as record(per_filter_noise=True)
        R = r((1.0 + np.arange(n) / n + 0.5 * (np.arange(n) % 3 == 0))[:, None, None] * R[None])
    earth = on.earth_rotation(sy.ORIENT_LATITUDE)
    mus, covs, ia, ib = [], [], [], []
    for c in range(steps):
        if model == "pose":
            acc, z, Q = sy.pose_cycle_inputs(n, c, mu[:, :3])
            acc[::5] = np.nan
            a, b = r(acc), np.zeros((n, 3))
        else:
            gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu[:, 0:4])
            a, b = r(acc), r(gyro)
        if c > 0:
            if model == "pose":
                mu, cov, s1 = capi.pose_predict(mu, cov, R, ia[-1], r(ACC_COV), float(dt[c - 1]), prec=prec)
                mu, cov, s2 = capi.pose_update(mu, cov, spe.MEAS_POS3, r(z), r(Q), prec=prec)
            else:
                mu, cov, s1 = capi.orient_predict(mu, cov, R, ia[-1], ib[-1], sy.ORIENT_TAU, sy.ORIENT_TAU, earth, float(dt[c - 1]),
                                                  prec=prec)
                mu, cov, s2 = capi.orient_update(mu, cov, r(z), r(Q), prec=prec)
            assert (s1 == 0).all() and (s2 == 0).all()
            mu, cov = r(mu), r(cov)
        mus.append(mu); covs.append(cov); ia.append(a); ib.append(b)
    if model == "pose":
        p = smr.Params("pose", R, acc_cov=r(2.0 * ACC_COV) / 2.0)
    else:
        p = smr.Params("orient", R, tau_g=sy.ORIENT_TAU, tau_a=sy.ORIENT_TAU, earth=earth)
    return p, np.array(mus), np.array(covs), dt, np.array(ia), np.array(ib)


def predicted_state(spe, model, n, prec=0):
    """the state of tests/test_gpu_innovation.make_engine (one prediction of the bench workload) by the C++ oracle, and its Q"""
    from oracle import capi, ukf_numpy as on
    sy = spe.synth
    r = sp.f32r if prec else (lambda x: np.asarray(x, dtype=np.float64))
    if model == "pose":
        mu, cov = sy.pose_initial(n)
        acc, _, Q = sy.pose_cycle_inputs(n, 0, mu[:, :3], random_q=True)
        mu, cov, st = capi.pose_predict(r(mu), r(cov), r(sy.pose_default_process_noise()), r(acc), r(ACC_COV), 0.01, prec=prec)
    else:
        mu, cov = sy.orient_initial(n)
        gyro, acc, _, Q = sy.orient_cycle_inputs(n, 0, mu[:, :4])
        G = sy.uniform(sy.SEED_BASE + 9, np.arange(n), np.arange(9), -1.0, 1.0).reshape(n, 3, 3)
        Q = 0.05 ** 2 * (np.eye(3)[None] + 0.3 * (G @ np.swapaxes(G, 1, 2)) / 3.0)
        Q = 0.5 * (Q + np.swapaxes(Q, 1, 2))
        mu, cov, st = capi.orient_predict(r(mu), r(cov), r(sy.orient_process_noise()), r(acc), r(gyro), sy.ORIENT_TAU, sy.ORIENT_TAU,
                                          on.earth_rotation(sy.ORIENT_LATITUDE), 0.01, prec=prec)
    assert (st == 0).all()
    return r(mu), r(cov), r(Q)
