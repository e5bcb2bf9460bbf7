"""Scale-aware parity: every block of the state is held to its own sigma.  A helper, not collected;
tests/test_scaled_parity_reference.py pins it, tests/test_gpu_scaled_parity.py and tools/scaled_parity_report.py use it.

The states the suite runs on are not of one scale (synth.ORIENT_DIAG_STD: variances 2.5e-3 orientation ... 1e-6 gyro bias), so
one absolute bound over all entries says nothing about the small blocks.  Here a result (mu, C) is measured against a reference
(mu_o, C_o) in the reference's own whitened metric, s_i = sqrt(C_o[i, i]):

    mean         |(mu (-) mu_o)_i| / s_i            (-) = the oracle's pose_boxminus / orient_boxminus
    covariance   |C - C_o|_ij / (s_i s_j)

and reduced to the max over filters and entries per mean block and per pair of covariance blocks (Pose 4 + 10 values,
OrientationState 5 + 15).  No filter is left out.

Bounds per block, u = 2^-24, m_i = max(1, |x_i|) over the stored scalars behind tangent coordinate i (2 for a rotation
coordinate), v = max m_i / s_i of a mean block, 1 for a covariance block:

    fp64 engine   1e-9
    wide fp32     2 c u v + 1e-9 against the fp64 oracle chain with the state rounded to fp32 at each of its c commits: one fp32
                  rounding per stored entry and commit, times 2 for ties that flip and are carried on.  A commit is counted where
                  consecutive SINGLE launches would write the state: once per cycle, also for the cycles of a multi-cycle
                  launch (its op list carries c commit markers).  The wide engine keeps the filter in fp64 between the cycles
                  of one launch and narrows once at its end (tests/test_gpu_wide_arithmetic.py), so engine and reference are
                  c + 1 roundings apart there, and c + 1 <= 2 c for every c >= 1
    fp32 engine   max(M d_o32, 20 u v), d_o32 = the same block's distance float oracle <-> fp64 oracle; the floor of 20 ulp is
                  FLOOR of tests/test_gpu_f32_horizon.py, in ulps of the value because two mean blocks are EXACTLY unchanged by a
                  prediction (Pose angular velocity, OrientationState gravity: d_o32 = 0 there)

M is measured on the CPU alone (profiles/scaled_parity.txt, recomputed by tests/test_scaled_parity_reference.py): twice the
largest per-block ratio between two independent correct fp32 evaluations of the algorithm, never from GPU results."""
import numpy as np

U = 2.0 ** -24
TOL_F64 = 1e-9
FLOOR_ULP = 20.0
# profiles/scaled_parity.txt ("M ="): 2 x the largest per-block spread between the C++ float oracle and the all-float32 NumPy
# evaluation (tests/study_f32_mixed.py), predict and predict + update of both bench workloads, 203 filters
M = 7.0

# model -> (blocks (name, tangent lo, hi), stored index behind each tangent coordinate; -1 = rotation coordinate)
BLOCKS = {
    "pose": (("position", 0, 3), ("orientation", 3, 6), ("velocity", 6, 9), ("angular_velocity", 9, 12)),
    "orient": (("orientation", 0, 3), ("velocity", 3, 6), ("gyro_bias", 6, 9), ("acc_bias", 9, 12), ("gravity", 12, 13)),
}
STORED = {
    "pose": np.array([0, 1, 2, -1, -1, -1, 7, 8, 9, 10, 11, 12]),
    "orient": np.array([-1, -1, -1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]),
}


def f32r(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def block_names(model):
    return [b[0] for b in BLOCKS[model]]


def boxminus(model, mu, mu_o):
    """[n, D]: mu (-) mu_o, filter by filter, with the oracle's own compound"""
    from oracle import capi
    f = capi.pose_boxminus if model == "pose" else capi.orient_boxminus
    return np.stack([f(a, b) for a, b in zip(np.asarray(mu, dtype=np.float64), np.asarray(mu_o, dtype=np.float64))])


class Dist:
    """mean [B], cov [B, B] (symmetric): the block maxima; mean_at / cov_at: the filter of each maximum"""

    def __init__(self, model, mean, cov, mean_at, cov_at):
        self.model, self.mean, self.cov, self.mean_at, self.cov_at = model, mean, cov, mean_at, cov_at

    def items(self):
        """(label, value, filter) for the B mean blocks and the B (B + 1) / 2 covariance block pairs"""
        names = block_names(self.model)
        out = [(f"mean[{a}]", self.mean[i], self.mean_at[i]) for i, a in enumerate(names)]
        for i, a in enumerate(names):
            for j in range(i, len(names)):
                out.append((f"cov[{a},{names[j]}]", self.cov[i, j], self.cov_at[i, j]))
        return out


def distances(model, mu, C, mu_o, C_o, filters=None):
    """Dist of (mu, C) from the reference (mu_o, C_o); `filters`: the batch index of each row, for the failure text"""
    mu, C, mu_o, C_o = (np.asarray(x, dtype=np.float64) for x in (mu, C, mu_o, C_o))
    n = mu.shape[0]
    filters = np.arange(n) if filters is None else np.asarray(filters)
    s = np.sqrt(np.einsum("nii->ni", C_o))
    dm = np.abs(boxminus(model, mu, mu_o)) / s
    dc = np.abs(C - C_o) / (s[:, :, None] * s[:, None, :])
    blocks = BLOCKS[model]
    B = len(blocks)
    mean, mean_at = np.zeros(B), np.zeros(B, dtype=np.int64)
    cov, cov_at = np.zeros((B, B)), np.zeros((B, B), dtype=np.int64)
    for i, (_, lo, hi) in enumerate(blocks):
        per = dm[:, lo:hi].max(axis=1)
        mean[i], mean_at[i] = per.max(), filters[per.argmax()]
        for j, (_, lo2, hi2) in enumerate(blocks):
            per = dc[:, lo:hi, lo2:hi2].reshape(n, -1).max(axis=1)
            cov[i, j], cov_at[i, j] = per.max(), filters[per.argmax()]
    return Dist(model, mean, cov, mean_at, cov_at)


def mean_scale(model, mu_o, C_o):
    """v [B]: the largest m_i / s_i of each mean block over the batch"""
    mu_o, C_o = np.asarray(mu_o, dtype=np.float64), np.asarray(C_o, dtype=np.float64)
    s = np.sqrt(np.einsum("nii->ni", C_o))
    idx = STORED[model]
    m = np.where(idx[None, :] < 0, 2.0, np.maximum(1.0, np.abs(mu_o[:, np.maximum(idx, 0)])))
    r = m / s
    return np.array([r[:, lo:hi].max() for _, lo, hi in BLOCKS[model]])


class Bound:
    def __init__(self, mean, cov):
        self.mean, self.cov = np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64)


def bound_f64(model):
    B = len(BLOCKS[model])
    return Bound(np.full(B, TOL_F64), np.full((B, B), TOL_F64))


def bound_wide(model, mu_o, C_o, commits):
    B = len(BLOCKS[model])
    return Bound(2.0 * commits * U * mean_scale(model, mu_o, C_o) + 1e-9, np.full((B, B), 2.0 * commits * U + 1e-9))


def floor_f32(model, mu_o, C_o):
    B = len(BLOCKS[model])
    return Bound(FLOOR_ULP * U * mean_scale(model, mu_o, C_o), np.full((B, B), FLOOR_ULP * U))


def bound_f32(model, mu_o, C_o, d_o32, margin=None):
    """d_o32: Dist of the float oracle from the fp64 oracle on the same inputs"""
    fl = floor_f32(model, mu_o, C_o)
    k = M if margin is None else margin
    return Bound(np.maximum(k * d_o32.mean, fl.mean), np.maximum(k * d_o32.cov, fl.cov))


def violations(dist, bound):
    """[(label, filter, value, bound)] of the blocks over their bound (a NaN is over every bound)"""
    names = block_names(dist.model)
    out = []
    for i, a in enumerate(names):
        if not dist.mean[i] <= bound.mean[i]:
            out.append((f"mean[{a}]", int(dist.mean_at[i]), float(dist.mean[i]), float(bound.mean[i])))
    for i, a in enumerate(names):
        for j in range(i, len(names)):
            if not dist.cov[i, j] <= bound.cov[i, j]:
                out.append((f"cov[{a},{names[j]}]", int(dist.cov_at[i, j]), float(dist.cov[i, j]), float(bound.cov[i, j])))
    return out


def check(dist, bound, what=""):
    bad = violations(dist, bound)
    assert not bad, f"{what}: " + "; ".join(f"block {b} filter {f}: {v:.3e} > bound {t:.3e}" for b, f, v, t in bad)


def table(dist, bound=None, other=None):
    """text rows: block, distance[, other distance][, bound]"""
    rows = []
    names = block_names(dist.model)
    B = len(names)
    for k, (label, v, f) in enumerate(dist.items()):
        row = f"  {label:38s} {v:10.3e}"
        if k < B:
            i = j = k
            pick = lambda x: x.mean[i]                                    # noqa: E731
        else:
            i, j = [(a, b) for a in range(B) for b in range(a, B)][k - B]
            pick = lambda x: x.cov[i, j]                                  # noqa: E731
        if other is not None:
            row += f" {pick(other):10.3e}"
        if bound is not None:
            row += f"   bound {pick(bound):10.3e}"
        rows.append(row)
    return "\n".join(rows)


# ------------------------------------------------------------------------------------------------ CPU: the fp32 spread behind M
SPREAD_N, SPREAD_DT = 203, 0.01


def bench_inputs(spe, workload, n=SPREAD_N, rounded=True):
    """the bench workload's state and first input set (BASELINE configs 3 / 4), as an fp32 engine holds them when `rounded`"""
    sy = spe.synth
    r = f32r if rounded else (lambda x: x)
    if workload == "pose":
        mu, cov = sy.pose_initial(n)
        acc, z, Q = sy.pose_cycle_inputs(n, 0, mu[:, :3])
        return dict(mu=r(mu), cov=r(cov), acc=r(acc), z=r(z), Q=r(Q), R=r(sy.pose_default_process_noise()),
                    acc_cov=r(0.01 * np.eye(3)))
    mu, cov = sy.orient_initial(n)
    gyro, acc, z, Q = sy.orient_cycle_inputs(n, 0, mu[:, :4])
    from oracle import ukf_numpy as onp
    return dict(mu=r(mu), cov=r(cov), gyro=r(gyro), acc=r(acc), z=r(z), Q=r(Q), R=r(sy.orient_process_noise()),
                earth=onp.earth_rotation(sy.ORIENT_LATITUDE), tau=sy.ORIENT_TAU)


def oracle_predict(spe, workload, i, mu, cov, prec=0, dt=SPREAD_DT, threads=1):
    from oracle import capi
    if workload == "pose":
        return capi.pose_predict(mu, cov, i["R"], i["acc"], i["acc_cov"], dt, prec=prec, threads=threads)
    return capi.orient_predict(mu, cov, i["R"], i["acc"], i["gyro"], i["tau"], i["tau"], i["earth"], dt, prec=prec, threads=threads)


def oracle_update(spe, workload, i, mu, cov, prec=0, threads=1):
    from oracle import capi
    if workload == "pose":
        return capi.pose_update(mu, cov, spe.MEAS_POS3, i["z"], i["Q"], prec=prec, threads=threads)
    return capi.orient_update(mu, cov, i["z"], i["Q"], prec=prec, threads=threads)


def numpy_f32_cycle(workload, i, dt=SPREAD_DT, kernel_ident=False):
    """((mu, C) after the prediction, (mu, C) after the update) of tests/study_f32_mixed.py with every stage float32"""
    import study_f32_mixed as st
    P = st.Prec("f32", st.F32, st.F32, st.F32, kernel_ident=kernel_ident)
    n = i["mu"].shape[0]
    m, c = i["mu"].astype(P.ts), i["cov"].astype(P.ts)
    bc = lambda a, X: (a[:, None, :] if X.ndim == 3 else a).astype(X.dtype)                    # noqa: E731
    if workload == "pose":
        R = i["R"].copy()
        R[6:9, 6:9] = 2.0 * i["acc_cov"]
        m, c = st.predict(st.POSE, m, c, lambda X: st.pose_process(X, bc(i["acc"], X), dt), np.broadcast_to(R, (n, 12, 12)), P, 6)
        m1, c1 = m.astype(P.ts), c.astype(P.ts)
        m, c = st.update(st.POSE, m1, c1, i["z"], lambda X: X[..., 0:3], i["Q"], P, linear_sel=[0, 1, 2])
    else:
        aff = np.ones(13)
        aff[6:12] = 1.0 - dt / i["tau"]
        proc = lambda X: st.orient_process(X, bc(i["acc"], X), bc(i["gyro"], X), i["tau"], i["earth"].astype(X.dtype), dt)   # noqa: E731
        m, c = st.predict(st.ORIENT, m, c, proc, np.broadcast_to(dt * dt * i["R"], (n, 13, 13)), P, 6, aff)
        m1, c1 = m.astype(P.ts), c.astype(P.ts)
        m, c = st.update(st.ORIENT, m1, c1, i["z"], lambda X: st.qrot(st.qinv(X[..., 0:4]), X[..., 4:7]), i["Q"], P)
    return (m1.astype(np.float64), c1.astype(np.float64)), (m.astype(P.ts).astype(np.float64), c.astype(P.ts).astype(np.float64))


def fp32_spread(spe, kernel_ident=False):
    """[(workload, stage, label, d float oracle, d NumPy f32, floor, ratio or None)], M: the spread between two independent
    correct fp32 evaluations, block by block, in the metric of this file; the statuses of all oracle runs must be 0"""
    rows, worst = [], 1.0
    for wl in ("pose", "orient"):
        i = bench_inputs(spe, wl)
        m64, c64, s = oracle_predict(spe, wl, i, i["mu"], i["cov"], 0)
        m32, c32, t = oracle_predict(spe, wl, i, i["mu"], i["cov"], 1)
        assert (s == 0).all() and (t == 0).all()
        n64 = (m64, c64)
        n32 = (m32, c32)
        u64 = oracle_update(spe, wl, i, m64, c64, 0)
        u32 = oracle_update(spe, wl, i, m32, c32, 1)
        assert (u64[2] == 0).all() and (u32[2] == 0).all()
        p_np, u_np = numpy_f32_cycle(wl, i, kernel_ident=kernel_ident)
        for stage, ref, a, b in (("predict", n64, n32, p_np), ("predict+update", u64[:2], u32[:2], u_np)):
            da, db = distances(wl, a[0], a[1], *ref), distances(wl, b[0], b[1], *ref)
            fl = floor_f32(wl, *ref)
            fa = [x for x in fl.mean] + [fl.cov[p, q] for p in range(len(fl.mean)) for q in range(p, len(fl.mean))]
            for (label, va, _), (_, vb, _), f in zip(da.items(), db.items(), fa):
                ratio = None
                if max(va, vb) > f:
                    ratio = max(va, vb) / max(min(va, vb), f)
                    worst = max(worst, ratio)
                rows.append((wl, stage, label, va, vb, f, ratio))
    return rows, 2.0 * worst


def spread_text(rows, m):
    out = ["# CPU: two fp32 evaluations of the algorithm against the fp64 oracle, whitened block distances (tests/scaled_parity.py)",
           f"# n = {SPREAD_N}, dt = {SPREAD_DT}, fp32-rounded synth inputs; ratio = larger / max(smaller, floor); '-' = both under the floor",
           f"# {'workload':8s} {'stage':15s} {'block':38s} {'float oracle':>12s} {'numpy f32':>12s} {'floor':>10s} {'ratio':>7s}"]
    for wl, stage, label, va, vb, f, r in rows:
        out.append(f"  {wl:8s} {stage:15s} {label:38s} {va:12.3e} {vb:12.3e} {f:10.3e} {('%7.2f' % r) if r else '      -'}")
    out.append(f"M = {m:.3f}   (2 x the largest ratio; the constant scaled_parity.M must not be smaller)")
    return "\n".join(out)


# ------------------------------------------------------------------------------------------------ input sets and reference chains
MODES = ("f64", "f32", "wide")          # fp64 engine, fp32 engine, fp32 engine with wide_arithmetic
ST_INACTIVE = 1 << 8                    # (engine.ST_INACTIVE: a filter without a sample in a launch; not an error)
THREADS = 8


class Case:
    """One batch as an engine of `mode` holds it: fp32 and wide engines round state, inputs, noise and Q to float (f32r).
    model "pose": acceleration NaN at [1::3] (both prediction branches inside each wavefront), a dense acceleration covariance,
    random per-filter Q; noise "default" (the ctor's / orient_process_noise: 1e-12 ... 1e-4) or "per_filter" (dense)."""

    def __init__(self, spe, model, mode, n=203, noise="default"):
        sy = spe.synth
        r = (lambda x: np.asarray(x, dtype=np.float64)) if mode == "f64" else f32r
        self.spe, self.model, self.mode, self.n, self.r = spe, model, mode, n, r
        if model == "pose":
            mu, cov = sy.pose_initial(n)
            acc, z, Q = sy.pose_cycle_inputs(n, 0, mu[:, :3], random_q=True)
            acc[1::3] = np.nan
            self.acc, self.acc_cov = r(acc), r(sy.dense_acc_cov())
            R = sy.pose_default_process_noise() if noise == "default" else sy.dense_process_noise_per_filter("pose", n)
        else:
            mu, cov = sy.orient_initial(n)
            gyro, acc, z, Q = sy.orient_cycle_inputs(n, 0, mu[:, :4])
            self.gyro, self.acc = r(gyro), r(acc)
            R = sy.orient_process_noise() if noise == "default" else sy.dense_process_noise_per_filter("orient", n)
            from oracle import ukf_numpy as onp
            self.earth, self.tau = onp.earth_rotation(sy.ORIENT_LATITUDE), sy.ORIENT_TAU
        self.mu, self.cov, self.z, self.Q, self.R = r(mu), r(cov), r(z), r(Q), r(R)
        self.full3 = spe.MEAS_POS3 if model == "pose" else spe.MEAS_ORIENT_BODYVEL3

    def z_for(self, models, k=0):
        """a measurement consistent with each filter's model id (Pose), shifted a little per cycle k"""
        if self.model != "pose":
            return self.r(self.z + 0.01 * k)
        mo = np.broadcast_to(np.asarray(models, dtype=np.int32), (self.n,))
        return self.r(self.spe.synth.pose_measurement_for_model(self.mu, mo, self.z - self.mu[:, :3] + 0.01 * k))

    def predict(self, mu, cov, dt, prec=0, R=None):
        from oracle import capi
        R = self.R if R is None else R
        if self.model == "pose":
            return capi.pose_predict(mu, cov, R, self.acc, self.acc_cov, dt, prec=prec, threads=THREADS)
        return capi.orient_predict(mu, cov, R, self.acc, self.gyro, self.tau, self.tau, self.earth, dt, prec=prec, threads=THREADS)

    def update(self, mu, cov, models, z, Q, prec=0):
        from oracle import capi
        if self.model == "pose":
            return capi.pose_update(mu, cov, models, z, Q, prec=prec, threads=THREADS)
        act = None if np.isscalar(models) else (np.asarray(models) >= 0)
        return capi.orient_update(mu, cov, z, Q, active=act, prec=prec, threads=THREADS)

    def chain(self, ops, prec=0, narrow=False, rows=None):
        """ops: ("predict", dt) | ("update", models, z, Q) | ("commit",): the engine writes the state to HBM here.  narrow: the
        state is rounded to float at every commit (the wide engine's reference).  rows: a subset of the filters.
        Returns mu, C, status (OR over the chain)."""
        sub = (lambda x: x) if rows is None else (lambda x: x[rows] if isinstance(x, np.ndarray) and x.ndim and x.shape[0] == self.n else x)
        keep = {k: getattr(self, k) for k in ("acc", "gyro", "R") if hasattr(self, k)}
        try:
            for k, v in keep.items():
                setattr(self, k, sub(v))
            m, c = sub(self.mu), sub(self.cov)
            st = np.zeros(m.shape[0], dtype=np.uint32)
            for op in ops:
                if op[0] == "commit":
                    if narrow:
                        m, c = f32r(m), f32r(c)
                    continue
                if op[0] == "predict":
                    m, c, s = self.predict(m, c, sub(op[1]), prec)
                else:
                    m, c, s = self.update(m, c, sub(op[1]), sub(op[2]), sub(op[3]), prec)
                st |= s
            return m, c, st
        finally:
            for k, v in keep.items():
                setattr(self, k, v)


def commits(ops):
    return sum(1 for op in ops if op[0] == "commit")


def judge(case, ops, mu_g, C_g, st_g, what="", rows=None, report=None):
    """The scaled check of an engine's result (mu_g, C_g, st_g: the rows `rows` of the batch, all of it by default) after the
    launches that `ops` describe.  Every filter counts; engine and oracles must agree on the status words and report no error
    (INACTIVE, a filter without a sample, is none).  report: a list that receives (what, Dist, Bound)."""
    model, mode = case.model, case.mode
    filters = np.arange(case.n) if rows is None else np.asarray(rows)
    m_o, c_o, st_o = case.chain(ops, 0, narrow=(mode == "wide"), rows=rows)
    assert (st_o & ~np.uint32(ST_INACTIVE) == 0).all(), f"{what}: fp64 oracle status {np.unique(st_o)}"
    assert (np.asarray(st_g) == st_o).all(), f"{what}: status differs from the oracle at filters {filters[np.nonzero(st_g != st_o)[0][:8]]}"
    d = distances(model, mu_g, C_g, m_o, c_o, filters)
    if mode == "f64":
        b = bound_f64(model)
    elif mode == "wide":
        b = bound_wide(model, m_o, c_o, commits(ops))
    else:
        m32, c32, st32 = case.chain(ops, 1, rows=rows)
        assert (st32 == st_o).all(), f"{what}: float oracle status {np.unique(st32)}"
        b = bound_f32(model, m_o, c_o, distances(model, m32, c32, m_o, c_o, filters))
    if report is not None:
        report.append((what, d, b))
    check(d, b, f"{what} [{mode} {model}]")
    return d, b
