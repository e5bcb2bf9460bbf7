"""NumPy float64 statement of the covariance conditioning of include/ukf_batch.h ("covariance conditioning"): the variance floor,
the correlation matrix, its eigendecomposition -- by numpy.linalg.eigh, or by a literal round-robin cyclic Jacobi with the
kernel's schedule, guard, threshold and sweep cap --, the verdict with its hysteresis, the additive repair, the optional
renormalisation of the quaternion and the status rules.  A helper, not collected; tests/test_condition_reference.py pins it."""
import numpy as np

from oracle import ukf_numpy as on

ST_REPAIRED = 1 << 11
MAX_SWEEPS = 12
U64, U32 = 2.0 ** -53, 2.0 ** -24


def quat_offset(man):
    """stored offset of the orientation quaternion"""
    return [f[1] for f in man.fields if f[0] == "so3"][0]


def schedule(D):
    """the round-robin (circle method) schedule: a list of steps, each a list of disjoint pairs (p, q), p < q < D.  D is rounded up
    to an even number of players DP, player DP - 1 is fixed; step r plays (DP - 1, r) and ((r + k) mod (DP - 1), (r - k) mod
    (DP - 1)), k = 1 ... DP / 2 - 1.  For an odd D player DP - 1 is a padding row decoupled from the rest: its pair is the
    identity (m_pq is an exact zero, the guard skips it) and is left out."""
    DP = (D + 1) // 2 * 2
    steps = []
    for r in range(DP - 1):
        pairs = [] if DP != D else [(min(DP - 1, r), max(DP - 1, r))]
        for k in range(1, DP // 2):
            a, b = (r + k) % (DP - 1), (r - k) % (DP - 1)
            pairs.append((min(a, b), max(a, b)))
        steps.append(pairs)
    return steps


def jacobi_eig(C, u=U64, max_sweeps=MAX_SWEEPS, dtype=np.float64):
    """C [B, D, D] symmetric -> (lam [B, D], V [B, D, D] with C = V diag(lam) V^T, converged [B], sweeps [B]).  In front of every
    sweep a matrix whose off-diagonal Frobenius norm (both triangles) is at most 4 D u is finished and is not rotated again; at
    most max_sweeps sweeps.  A step rotates its disjoint pairs at once, M <- J^T (M J), V <- V J, every (c, s) from m_pp, m_qq and
    m_pq as row p holds them; a pair with |m_pq| <= u is not rotated.  dtype = numpy.float32 with u = U32 is the all-float32
    emulation of the fp32 kernel."""
    M = np.array(C, dtype=dtype)
    B, D = M.shape[0], M.shape[1]
    V = np.broadcast_to(np.eye(D, dtype=dtype), (B, D, D)).copy()
    lam, Vout = np.full((B, D), np.nan, dtype=dtype), np.full((B, D, D), np.nan, dtype=dtype)
    done, conv, sweeps = np.zeros(B, bool), np.zeros(B, bool), np.zeros(B, dtype=np.int64)
    offd = ~np.eye(D, dtype=bool)
    steps = schedule(D)
    for sw in range(max_sweeps + 1):
        off2 = np.sum(np.where(offd, M, dtype(0)) ** 2, axis=(1, 2))
        with np.errstate(invalid="ignore"):
            newly = ~done & (off2 <= dtype((4.0 * D * u) ** 2))
        lam[newly], Vout[newly] = np.einsum("bii->bi", M)[newly], V[newly]
        conv |= newly
        done |= newly
        if sw == max_sweeps or done.all():
            break
        act = np.nonzero(~done)[0]
        sweeps[act] += 1
        Ma, Va = M[act], V[act]
        for pairs in steps:
            J = np.broadcast_to(np.eye(D, dtype=dtype), (act.size, D, D)).copy()
            for p, q in pairs:
                a, b, x = Ma[:, p, p], Ma[:, q, q], Ma[:, p, q]
                with np.errstate(all="ignore"):
                    one = dtype(1)
                    rot = np.abs(x) > dtype(u)
                    xs = np.where(rot, x, one)
                    th = (b - a) / (dtype(2) * xs)
                    t = np.copysign(one, th) / (np.abs(th) + np.sqrt(th * th + one))
                    cc = one / np.sqrt(t * t + one)
                c, s = np.where(rot, cc, one), np.where(rot, t * cc, dtype(0))
                J[:, p, p], J[:, q, q], J[:, p, q], J[:, q, p] = c, c, s, -s
            with np.errstate(all="ignore"):
                Ma = np.swapaxes(J, 1, 2) @ (Ma @ J)
                Va = Va @ J
        M[act], V[act] = Ma, Va
    return lam, Vout, conv, sweeps


def correlation(cov, var_floor):
    """-> (C [B, D, D] with unit diagonal, s [B, D], d [B, D], raised [B]) of steps 2 and 3; the lower triangle is what is read"""
    D = cov.shape[1]
    low = np.tril(cov)
    sym = low + np.swapaxes(np.tril(cov, -1), 1, 2)
    diag = np.einsum("bii->bi", cov)
    with np.errstate(invalid="ignore"):
        raised = diag < var_floor
        d = np.where(raised, var_floor, diag)
        s = np.sqrt(d)
        C = sym / (s[:, :, None] * s[:, None, :])
    C[:, np.arange(D), np.arange(D)] = 1.0
    return C, s, d, raised.any(axis=1)


def repair(C, lam, V, eig_floor):
    """C' = C + sum_{k: lambda_k < eps} (eps - lambda_k) v_k v_k^T"""
    w = np.where(lam < eig_floor, eig_floor - lam, 0.0)
    return C + np.einsum("bk,bik,bjk->bij", w, V, V)


def condition(man, mu, cov, var_floor, eig_floor, select=None, initialised=None, renormalize=False, method="eigh", u_storage=U64):
    """mu [B, S], cov [B, D, D], var_floor [D] -> dict(mu, cov: the state after a committing call; eig_min, eig_max [B] (NaN
    where the call reports a failure), status [B], sweeps [B] (method "jacobi")).  u_storage: the unit roundoff of the storage type
    whose rounding decides whether a quaternion is already unit."""
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    B, D = mu.shape[0], man.D
    v = np.asarray(var_floor, dtype=np.float64).reshape(D)
    init = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    sel = np.ones(B, bool) if select is None else np.asarray(select) != 0
    o = {"mu": mu.copy(), "cov": cov.copy(), "eig_min": np.full(B, np.nan), "eig_max": np.full(B, np.nan),
         "status": np.zeros(B, dtype=np.uint32), "sweeps": np.zeros(B, dtype=np.int64)}
    o["status"][~init] = on.ST_UNINITIALISED
    o["status"][init & ~sel] = on.ST_INACTIVE
    todo = init & sel
    if not (np.isfinite(v).all() and (v > 0).all()):
        o["status"][todo] = on.ST_ERR_NONFINITE_MEAS
        return o
    lower = np.tril(np.ones((D, D), bool))
    fin = np.isfinite(cov[:, lower]).all(axis=1)
    Q = quat_offset(man)
    q = mu[:, Q:Q + 4]
    n2 = q[:, 3] * q[:, 3] + (q[:, 2] * q[:, 2] + (q[:, 1] * q[:, 1] + q[:, 0] * q[:, 0]))
    with np.errstate(invalid="ignore"):
        qbad = ~(np.isfinite(n2) & (n2 > 0.0)) if renormalize else np.zeros(B, bool)
        qmove = (np.abs(n2 - 1.0) > 8.0 * u_storage) if renormalize else np.zeros(B, bool)
    ok = todo & fin & ~qbad
    o["status"][todo & ~ok] = on.ST_ERR_CHOLESKY
    idx = np.nonzero(ok)[0]
    if idx.size == 0:
        return o
    C, s, d, raised = correlation(cov[idx], v)
    if method == "eigh":
        lam, V = np.linalg.eigh(C)
        conv = np.ones(idx.size, bool)
    else:
        lam, V, conv, o["sweeps"][idx] = jacobi_eig(C)
    o["status"][idx[~conv]] = on.ST_ERR_CHOLESKY
    idx, C, s, d, raised, lam, V = idx[conv], C[conv], s[conv], d[conv], raised[conv], lam[conv], V[conv]
    emin, emax = lam.min(axis=1), lam.max(axis=1)
    o["eig_min"][idx], o["eig_max"][idx] = emin, emax
    fix = raised | (emin < 0.5 * eig_floor)
    Cn = repair(C[fix], lam[fix], V[fix], eig_floor)
    Sn = Cn * (s[fix][:, :, None] * s[fix][:, None, :])
    Sn[:, np.arange(D), np.arange(D)] = d[fix] * np.einsum("bii->bi", Cn)   # never below the floor: C'_ii >= 1
    Sn = np.tril(Sn) + np.swapaxes(np.tril(Sn, -1), 1, 2)                   # the lower triangle is what is stored
    o["cov"][idx[fix]] = Sn
    rq = qmove[idx]
    o["mu"][idx[rq], Q:Q + 4] = q[idx[rq]] * (1.0 / np.sqrt(n2[idx[rq]]))[:, None]
    o["status"][idx[fix | rq]] = ST_REPAIRED
    return o


def correlation_eigen(cov):
    """-> (lam [B, D] ascending, V, s [B, D]) of the correlation matrix of cov with its own diagonal"""
    s = np.sqrt(np.einsum("bii->bi", cov))
    lam, V = np.linalg.eigh(cov / (s[:, :, None] * s[:, None, :]))
    return lam, V, s


def with_eigenvalues(cov, targets):
    """cov [B, D, D] positive definite, targets: a list of values for the smallest eigenvalues of the correlation matrix ->
    cov' with the sigmas of cov whose correlation matrix has unit diagonal and (to first order in the change of its diagonal)
    the smallest eigenvalues replaced by `targets`: V diag(lam') V^T is rescaled to unit diagonal, twice over, so that the
    eigenvalues that come out sit within a few percent of the targets."""
    lam, V, s = correlation_eigen(cov)
    D = cov.shape[1]
    want = lam.copy()
    want[:, :len(targets)] = np.asarray(targets, dtype=np.float64)
    C = np.einsum("bik,bk,bjk->bij", V, want, V)
    for _ in range(2):
        g = 1.0 / np.sqrt(np.einsum("bii->bi", C))
        C = C * (g[:, :, None] * g[:, None, :])
        l2, V2 = np.linalg.eigh(C)
        l2[:, :len(targets)] = np.asarray(targets, dtype=np.float64)
        C = np.einsum("bik,bk,bjk->bij", V2, l2, V2)
    g = 1.0 / np.sqrt(np.einsum("bii->bi", C))
    C = C * (g[:, :, None] * g[:, None, :])
    C = 0.5 * (C + np.swapaxes(C, 1, 2))
    C[:, np.arange(D), np.arange(D)] = 1.0
    return C * (s[:, :, None] * s[:, None, :])


def make_batch(cov, eig_floor, dtype, seed=23):
    """The four quarters of the GPU tests from healthy covariances cov [B, D, D]: -> (cov' [B, D, D] rounded to `dtype`, var_floor
    [D] rounded to `dtype`, quarter [B]).  Quarter 0 is untouched; 1 has lambda_min = -1e-3; 2 has its two smallest eigenvalues at
    -0.3 and -0.05; 3 has lambda_min = eps / 8 and one diagonal entry (t = filter index mod D) below the floor: row and column t
    are scaled so that the variance IS the floor v_t -- the correlation matrix keeps its eigenvalues -- and the stored diagonal
    entry is then v_t / 4, which the floor raises back.  The floor is 1e-3 of the smallest variance of each dimension in the batch.
    The quarters are dealt by a seeded permutation: wavefronts of one kind and mixed ones both occur."""
    B, D = cov.shape[0], cov.shape[1]
    stored = lambda x: np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)   # noqa: E731
    quarter = np.random.default_rng(seed).permutation(B) % 4
    v = stored(1e-3 * np.einsum("bii->bi", cov).min(axis=0))
    out = cov.copy()
    for k, targets in ((1, [-1e-3]), (2, [-0.3, -0.05]), (3, [eig_floor / 8.0])):
        out[quarter == k] = with_eigenvalues(cov[quarter == k], targets)
    for b in np.nonzero(quarter == 3)[0]:
        t = b % D
        g = np.ones(D)
        g[t] = np.sqrt(v[t] / out[b, t, t])
        out[b] = out[b] * np.outer(g, g)
        out[b, t, t] = v[t] / 4.0
    return stored(out), v, quarter
