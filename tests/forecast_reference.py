"""NumPy statement of the forecast of include/ukf_batch.h ("forecast"): `steps` predictions chained from a start record, each
made as ukfb_predict makes it, without an engine.  Built from oracle.ukf_numpy (ukf_predict, gate_dt, gate_timestamps) and
the process models and noise shaping of tests/smoother_reference.py (Params, _process_and_noise).  A helper, not collected;
tests/test_forecast_reference.py pins it.

Arrays are in WINDOW order (step c = the state after c + 1 predictions): mu [steps, B, S], cov [steps, B, D, D]; dt [steps]
(every filter's time step) or ts_us [steps] with last_us [B] (stamps against every filter's own last measurement time, the
chain of oracle.ukf_numpy.gate_timestamps); the optional inputs in_a / in_b are [steps, B, 3] (step c's row serves the
prediction that produces step c) or [B, 3] (latched, held over the horizon).

prec = "f64": the float64 reference, the oracle's own ukf_predict per step.  prec = "f32": the all-float32 evaluation of the
same call with the stage functions of tests/study_f32_mixed.py (as tests/feature_f32.py evaluates the other features), the
d_32 of tests/feature_scaled_parity.py: the start record in float32, the chain never narrowed below the arithmetic dtype,
every step's record rounded once.  It computes every row it predicts and expects covariances that factorise."""
import copy

import numpy as np

from oracle import ukf_numpy as on
import smoother_reference as sr

GATED = on.ST_SKIPPED_FIRST_TS | on.ST_SKIPPED_SMALL_DT | on.ST_ERR_NEG_DT | on.ST_ERR_DT_TOO_LARGE


def _rows(p, idx):
    """p for the filters idx (a process noise per filter is per row)"""
    q = copy.copy(p)
    if np.ndim(p.R) == 3:
        q.R = p.R[idx]
    return q


def _predict_f64(p, mu, cov, dt, a, b):
    g, R = sr._process_and_noise(p, mu, dt, a, b)
    with np.errstate(all="ignore"):
        return on.ukf_predict(p.man, mu, cov, g, R, p.mean_tol, p.mean_max_it)


def _predict_staged(p, mu, cov, dt, a, b, P):
    """one prediction with a dtype per stage: (mu in tc, cov in tl) -> (mu in tc, cov in tl)"""
    import feature_f32 as ff
    import study_f32_mixed as st
    model, B = p.model, mu.shape[0]
    _, R = sr._process_and_noise(p, mu.astype(np.float64), dt, a, b)
    bc = lambda v, X: (v[:, None, :] if X.ndim == 3 else v).astype(X.dtype)   # noqa: E731
    if model == "pose":
        use = np.zeros(B, bool) if a is None else np.isfinite(a).all(axis=-1)
        acc = np.where(use[:, None], np.zeros((B, 3)) if a is None else a, 0.0)
        g = lambda X: st.pose_process(X, bc(acc, X), dt)                     # noqa: E731
    else:
        assert p.tau_g == p.tau_a
        g = lambda X: st.orient_process(X, bc(a, X), bc(b, X), p.tau_g, p.earth.astype(X.dtype), dt)   # noqa: E731
    m, C = st.predict(ff.STATE[model], mu, cov, g, R, P)
    return m, C, np.zeros(B, dtype=np.uint32)


def forecast(p, mu0, cov0, dt=None, ts_us=None, last_us=None, in_a=None, in_b=None, initialised=None, prec="f64"):
    """-> (mu [steps, B, S], cov [steps, B, D, D], status [B], status_steps [steps, B]).  Uninitialised filters keep NaN in
    the outputs (nothing is written for them) and report UNINITIALISED.  A step that is gated or whose covariance does not
    factorise is the record before it, bit for bit (step 0: the start record)."""
    assert (dt is None) != (ts_us is None), "exactly one of dt / ts_us"
    staged = prec != "f64"
    if staged:
        import feature_f32 as ff
        P = ff.PRECISIONS[prec]
        m, C = np.asarray(mu0, dtype=np.float64).astype(P.ts).astype(P.tc), np.asarray(cov0, dtype=np.float64).astype(P.ts).astype(P.tl)
        out = lambda x: x.astype(P.ts).astype(np.float64)   # noqa: E731
    else:
        m, C = np.array(mu0, dtype=np.float64), np.array(cov0, dtype=np.float64)
        out = lambda x: x.copy()   # noqa: E731
    B = m.shape[0]
    steps = len(dt) if dt is not None else len(ts_us)
    if ts_us is not None:
        ts_us = np.asarray(ts_us, dtype=np.int64).reshape(steps)
        last = np.array(np.broadcast_to(np.asarray(last_us, dtype=np.int64), (B,)))
    else:
        dt = np.asarray(dt, dtype=np.float64).reshape(steps)
    ring = lambda x, c: None if x is None else (x[c] if np.ndim(x) == 3 else x)   # noqa: E731
    mus, covs = np.empty((steps,) + m.shape), np.empty((steps,) + C.shape)
    sts = np.zeros((steps, B), dtype=np.uint32)
    for c in range(steps):
        if ts_us is not None:
            last, d, gate = on.gate_timestamps(np.full(B, ts_us[c]), last, p.min_dt, p.max_dt)
        else:
            d = np.full(B, dt[c])
            gate = on.gate_dt(d, p.min_dt, p.max_dt)
        sts[c] = gate
        a, b = ring(in_a, c), ring(in_b, c)
        go = gate == 0
        for v in np.unique(d[go]):   # one prediction per distinct time step (one in the dt form)
            idx = np.nonzero(go & (d == v))[0]
            sub = lambda x: None if x is None else x[idx]   # noqa: E731
            if staged:
                mi, Ci, si = _predict_staged(_rows(p, idx), m[idx], C[idx], float(v), sub(a), sub(b), P)
            else:
                mi, Ci, si = _predict_f64(_rows(p, idx), m[idx], C[idx], float(v), sub(a), sub(b))
            m[idx], C[idx], sts[c, idx] = mi, Ci, si   # (ukf_predict: a row that does not factorise comes back as it went in)
        mus[c], covs[c] = out(m), out(C)
    status = np.bitwise_or.reduce(sts, axis=0)
    if initialised is not None:
        dead = ~np.asarray(initialised, dtype=bool)
        mus[:, dead], covs[:, dead] = np.nan, np.nan
        status = np.where(dead, on.ST_UNINITIALISED, status).astype(np.uint32)
    return mus, covs, status.astype(np.uint32), sts
