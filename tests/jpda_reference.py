"""NumPy float64 statement of include/ukf_batch_jpda.h: the exact joint association marginals of a scene by the subset
recurrences the kernel runs (F forward, G backward over the subsets of the scene's tracks), brute_force over every joint event
to hold them to, the launch over the scenes of an engine (jpda_scenes), and the update with given weights (update_weighted),
made of pda_reference's pieces: update_reference.scored_update, combine_textbook, on.apply_delta.  Also the inputs of the GPU
tests: the synthetic scores of tests/test_gpu_jpda.py and the constructed scenes of the end-to-end test.  A helper, not
collected; tests/test_jpda_reference.py pins it."""
import itertools

import numpy as np

import pda_reference as pr
import sensor_meas_reference as sr
from oracle import ukf_numpy as on
from update_reference import scored_update

MAX_TRACKS = 6
MAX_SEGMENT = 32           # a longer segment is a BAD scene (the assignment's segment rule), 7 ... 32 tracks a TOO_LARGE one
MAX_CANDIDATES = 32
LOG_RATIO_MAX = 100.0
OK, BAD_SCENE, TOO_LARGE = 0, 1, 2
FAILED = pr.FAILED


# ------------------------------------------------------------------------------------------------------------ one scene
def pair_rules(loglik, maha, gate):
    """loglik, maha [T, K] (maha None without a gate) -> (allowed, scored) [T, K]"""
    loglik = np.asarray(loglik, dtype=np.float64)
    scored = np.isfinite(loglik)
    allowed = scored.copy()
    if gate >= 0.0:
        maha = np.asarray(maha, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            allowed &= np.isfinite(maha) & (np.where(np.isfinite(maha), maha, np.inf) <= gate)
    return allowed, scored


def log_ratio(loglik, a0, ln_pd):
    """l_ik = (ln P_D + loglik) - a_0(m_i), in that order, in float64 (anything where loglik is not finite)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (ln_pd + np.asarray(loglik, dtype=np.float64)) - np.asarray(a0, dtype=np.float64)[:, None]


def psi_of(loglik, maha, gate, a0, ln_pd):
    """-> (psi [T, K]: exp(min(l, 100)) on the allowed pairs, 0 elsewhere; allowed; scored)"""
    allowed, scored = pair_rules(loglik, maha, gate)
    l = np.where(allowed, log_ratio(np.where(allowed, loglik, 0.0), a0, ln_pd), 0.0)
    return np.where(allowed, np.exp(np.minimum(l, LOG_RATIO_MAX)), 0.0), allowed, scored


def marginals(psi):
    """psi [T, K] -> (beta [T, K], beta0 [T], Z) by the subset recurrences: with S a bitmask over the tracks,
    F_{k+1}[S] = F_k[S] + sum_{i in S} psi_ik F_k[S ^ 2^i] (F_0 = [S empty]), G_k[U] = G_{k+1}[U] + sum_{i not in U} psi_ik
    G_{k+1}[U ^ 2^i] (G_K = 1), Z = G_0[0], beta_ik = sum_{S without i} F_k[S] psi_ik G_{k+1}[S ^ 2^i] / Z, beta_i0 =
    sum_{S without i} F_K[S] / Z"""
    psi = np.asarray(psi, dtype=np.float64)
    T, K = psi.shape
    sub = np.arange(1 << T)
    has = [((sub >> i) & 1).astype(bool) for i in range(T)]
    G = np.ones((K + 1, 1 << T))
    state = np.seterr(over="ignore", invalid="ignore")   # (products the selects below discard may overflow at the cap)
    for k in range(K - 1, -1, -1):
        g = G[k + 1].copy()
        for i in range(T):
            g += np.where(has[i], 0.0, psi[i, k] * G[k + 1][sub ^ (1 << i)])
        G[k] = g
    Z = G[0][0]
    F = np.zeros(1 << T)
    F[0] = 1.0
    beta = np.zeros((T, K))
    for k in range(K):
        nf = F.copy()
        for i in range(T):
            beta[i, k] = np.where(has[i], 0.0, F * (psi[i, k] * G[k + 1][sub ^ (1 << i)])).sum() / Z
            nf += np.where(has[i], psi[i, k] * F[sub ^ (1 << i)], 0.0)
        F = nf
    beta0 = np.array([np.where(has[i], 0.0, F).sum() / Z for i in range(T)])
    np.seterr(**state)
    return beta, beta0, Z


def brute_force(psi):
    """the definition: every joint event (each track one allowed detection or none, no detection twice), weight = product of psi"""
    psi = np.asarray(psi, dtype=np.float64)
    T, K = psi.shape
    beta, beta0, Z = np.zeros((T, K)), np.zeros(T), 0.0
    choices = [[-1] + [k for k in range(K) if psi[i, k] > 0.0] for i in range(T)]
    for pick in itertools.product(*choices):
        taken = [k for k in pick if k >= 0]
        if len(set(taken)) != len(taken):
            continue
        w = 1.0
        for i, k in enumerate(pick):
            if k >= 0:
                w *= psi[i, k]
        Z += w
        for i, k in enumerate(pick):
            if k >= 0:
                beta[i, k] += w
            else:
                beta0[i] += w
    return beta / Z, beta0 / Z, Z


# ------------------------------------------------------------------------------------------------------------ the launch
def segment_status(a, b, capacity):
    if not (a >= 0 and b <= capacity and b >= a and b - a <= MAX_SEGMENT):
        return BAD_SCENE
    return TOO_LARGE if b - a > MAX_TRACKS else OK


def rounded_logs(rule, dtype):
    """(a_0 for m = 1, a_0 for m = 3, ln P_D) as the launch hands them to the kernel: formed in double, rounded to the engine's
    storage type"""
    a0, ln_pd = pr.log_terms(rule, np.array([1, 3]))
    r = lambda x: float(np.asarray(x, dtype=np.float64).astype(dtype))   # noqa: E731
    return r(a0[0]), r(a0[1]), r(ln_pd)


def jpda_scenes(man, loglik, maha, scene_start, models, rule=pr.RULE, gate=-1.0, dtype=np.float64, sentinel=-7.0):
    """The launch: loglik, maha [K, capacity] as the engine stores them (maha None without a gate), scene_start [scenes + 1],
    models an id or [capacity].  -> dict: beta [K, capacity] and beta0 [capacity] in float64 before the store's rounding
    (`sentinel` where nothing is written), free [scenes, K], log_z [scenes] (sentinel on a scene that is not solved),
    scene_status [scenes]"""
    loglik = np.asarray(loglik, dtype=np.float64)
    K, cap = loglik.shape
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (cap,))
    a0_m1, a0_m3, ln_pd = rounded_logs(rule, dtype)
    a0 = np.where(pr.kernel_dim(man, models) == 1, a0_m1, a0_m3)
    scenes = len(scene_start) - 1
    out = {"beta": np.full((K, cap), sentinel), "beta0": np.full(cap, sentinel), "free": np.full((scenes, K), sentinel),
           "log_z": np.full(scenes, sentinel), "scene_status": np.zeros(scenes, dtype=np.uint32)}
    for s in range(scenes):
        a, b = int(scene_start[s]), int(scene_start[s + 1])
        out["scene_status"][s] = segment_status(a, b, cap)
        if out["scene_status"][s] != OK:
            continue
        psi, allowed, scored = psi_of(loglik[:, a:b].T, None if maha is None else maha[:, a:b].T, gate, a0[a:b], ln_pd)
        beta, beta0, Z = marginals(psi)
        out["beta"][:, a:b] = np.where(scored, np.where(allowed, beta, 0.0), np.nan).T
        out["beta0"][a:b] = beta0
        out["free"][s] = 1.0 - beta.sum(axis=0)
        out["log_z"][s] = np.log(Z)
    return out


def uniform_starts(capacity, tracks_per_scene, scenes=None):
    n = -(-capacity // tracks_per_scene) if scenes is None else scenes
    return np.minimum(np.arange(n + 1, dtype=np.int64) * tracks_per_scene, capacity).astype(np.int32)


def covered(scene_start, capacity):
    """the slots a launch writes: those of its OK scenes"""
    mask = np.zeros(capacity, dtype=bool)
    for a, b in zip(scene_start[:-1], scene_start[1:]):
        if segment_status(int(a), int(b), capacity) == OK:
            mask[a:b] = True
    return mask


# ------------------------------------------------------------------------------------- the synthetic inputs of the GPU tests
RAGGED_SIZES = (0, 1, 2, 3, 4, 5, 6)
SYNTH_GATE = 12.0


def ragged_starts(capacity, first=5):
    """scene sizes cycling through 0 ... 6 from slot `first` (with four scenes to a workgroup every size meets every position);
    the last scene ends at capacity"""
    starts, at, i = [first], first, 0
    while at < capacity:
        at = min(at + RAGGED_SIZES[i % len(RAGGED_SIZES)], capacity)
        starts.append(at)
        i += 1
    return np.array(starts, dtype=np.int32)


def synthetic_scores(seed, capacity, K, dtype):
    """-> (loglik, maha) [K, capacity] as an engine of `dtype` stores them: maha = d^2 in [0, 20), loglik = -d^2 / 2 - c with c in
    [-1, 7) per pair, so that l = ln P_D + loglik - a_0 spans about -18 ... +5 around the rule's a_0; 20 % of the pairs NaN,
    +inf or -inf in loglik, a further 5 % NaN in maha alone"""
    rng = np.random.default_rng(seed)
    d2 = rng.uniform(0.0, 20.0, size=(K, capacity))
    ll = -0.5 * d2 - rng.uniform(-1.0, 7.0, size=(K, capacity))
    bad = rng.random((K, capacity))
    ll[bad < 0.10] = np.nan
    ll[(bad >= 0.10) & (bad < 0.15)] = np.inf
    ll[(bad >= 0.15) & (bad < 0.20)] = -np.inf
    d2[(bad >= 0.20) & (bad < 0.25)] = np.nan
    return ll.astype(dtype).astype(np.float64), d2.astype(dtype).astype(np.float64)


def mixed_models(man, capacity):
    """sensor ids cycling through the engine's own (m = 1 and m = 3 for Pose), -1 and an id of the other engine"""
    own = list(sr.ids_of(man))
    other = [i for i in range(8) if i not in own][:1]
    ids = own + [-1] + other
    return np.array([ids[i % len(ids)] for i in range(capacity)], dtype=np.int32)


def largest_log_ratio(loglik, models, man, rule, dtype, maha=None, gate=-1.0):
    """max |l| over the ALLOWED pairs of a launch (l is formed for no other): the tests assert it below LOG_RATIO_MAX"""
    a0_m1, a0_m3, ln_pd = rounded_logs(rule, dtype)
    a0 = np.where(pr.kernel_dim(man, np.broadcast_to(models, loglik.shape[1:])) == 1, a0_m1, a0_m3)
    allowed, _ = pair_rules(loglik, maha, gate)
    l = (ln_pd + np.where(allowed, loglik, 0.0)) - a0[None, :]
    return float(np.abs(l[allowed]).max())


# ------------------------------------------------------------------------------------------- the update with given weights
def update_weighted(man, mu, cov, models, z, Q, mount, point, weight, gyro=None, initialised=None, commit=True, tol=on.MEAN_TOL,
                    max_it=on.MEAN_MAX_IT, dtype=np.float64):
    """-> dict(mu, cov, z_pred [B, 3], S [B, 3, 3], innov [K, B, 3], maha, loglik, weight_used [K, B], beta0 [B], innov_comb
    [B, 3], n_used [B], status [B]).  weight [K, B]; cfg.gate_chi2 plays no part."""
    z = np.asarray(z, dtype=np.float64)
    weight = np.asarray(weight, dtype=np.float64)
    K, B = z.shape[0], z.shape[1]
    D = man.D
    models = np.broadcast_to(np.asarray(models, dtype=np.int64), (B,))
    Q = np.broadcast_to(np.asarray(Q, dtype=np.float64), (B, 3, 3))
    mount = np.broadcast_to(np.asarray(mount, dtype=np.float64), (B, 7))
    point = np.broadcast_to(np.asarray(point, dtype=np.float64), (B, 3))
    gyro = np.zeros((B, 3)) if gyro is None else np.asarray(gyro, dtype=np.float64)
    init = np.ones(B, bool) if initialised is None else np.asarray(initialised, dtype=bool)
    valid = np.isin(models, sr.ids_of(man))
    mk = pr.kernel_dim(man, models)
    lead = np.arange(3)[None, :] < mk[:, None]
    nanf = lambda *s: np.full(s, np.nan)   # noqa: E731
    o = {"mu": mu.copy(), "cov": cov.copy(), "z_pred": nanf(B, 3), "S": nanf(B, 3, 3), "innov": nanf(K, B, 3), "maha": nanf(K, B),
         "loglik": nanf(K, B), "weight_used": nanf(K, B), "beta0": nanf(B), "innov_comb": nanf(B, 3)}
    o["innov"][:, ~lead] = 0.0
    o["innov_comb"][~lead] = 0.0
    n_used = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.uint32)
    status[~init] = on.ST_UNINITIALISED
    status[init & ~valid] = on.ST_INACTIVE
    for mid in np.unique(models[init & valid]):
        mid = int(mid)
        m = sr.meas_dim(mid)
        idx = np.nonzero(init & valid & (models == mid))[0]
        _, uq, um, up = sr.used_inputs(mid)
        fin = (np.isfinite(Q[idx][:, uq]).all(axis=1) & np.isfinite(mount[idx][:, um]).all(axis=1) & np.isfinite(point[idx][:, up]).all(axis=1))
        present = np.isfinite(z[:, idx, :m]).all(axis=2)
        go = fin & present.any(axis=0)
        status[idx[~go]] = on.ST_ERR_NONFINITE_MEAS
        idx, present = idx[go], present[:, go]
        if idx.size == 0:
            continue
        n = idx.size
        manz = on.VECT(m)
        mt = np.where(um, mount[idx], sr.IDENTITY_MOUNT)[:, None, :]
        pt = np.where(up, point[idx], 0.0)[:, None, :]
        gy = gyro[idx][:, None, :]
        hh = lambda X: sr.h(mid, X, mt, pt, gy)   # noqa: E731
        zz = np.where(present[:, :, None], z[:, idx, :m], 0.0)
        z_any = zz[np.argmax(present, axis=0), np.arange(n)]
        u = scored_update(man, manz, mu[idx], cov[idx], z_any, hh, Q[idx][:, :m, :m], tol, max_it, 0.0)
        X, _ = on.sigma_points(man, mu[idx], cov[idx])
        C = on.cross_cov_sigma_points(man, manz, mu[idx], u.mz, X, u.Z)
        S = np.where(u.scored[:, None, None], u.S, np.eye(m))
        Si = np.linalg.inv(S)
        Kg = C @ Si
        nu = zz - u.mz[None]
        with np.errstate(over="ignore", invalid="ignore"):
            d2 = np.einsum("kbi,bij,kbj->kb", nu, Si, nu)
        loglik = -0.5 * (d2 + u.logdet[None] + m * sr.LN_2PI)
        scored = u.scored[None] & present
        finite = scored & np.isfinite(d2)
        # ---- the weights: read, not computed
        w = weight[:, idx]
        with np.errstate(invalid="ignore"):
            used = finite & np.isfinite(w) & (np.where(np.isfinite(w), w, 0.0) > 0.0)
        wk = np.where(used, w, 0.0).astype(dtype)
        s = wk.sum(axis=0, dtype=dtype)
        c = np.maximum(dtype(1), s)
        beta = (wk / c[None]).astype(dtype)
        beta0 = (dtype(1) - s / c).astype(dtype)
        nu_used = np.where(used[:, :, None], nu, 0.0)
        accept = used.any(axis=0)
        cov2, delta, nub = pr.combine_textbook(cov[idx], Kg, S, nu_used, beta, beta0, dtype)
        cov2 = np.where((u.scored & accept)[:, None, None], cov2.astype(np.float64), np.eye(D))
        m2, C2, ok2 = on.apply_delta(man, mu[idx], cov2, np.where(accept[:, None], delta.astype(np.float64), 0.0))
        okc = u.scored & (ok2 | ~accept)
        st = np.where(okc, 0, on.ST_ERR_CHOLESKY).astype(np.uint32)
        st |= np.where(u.ok & ((u.status & on.ST_WARN_MEAN_NOCONV) != 0), on.ST_WARN_MEAN_NOCONV, 0).astype(np.uint32)
        st |= np.where(okc & finite.any(axis=0) & ~accept, on.ST_REJECTED_GATE, 0).astype(np.uint32)
        status[idx] = st
        s_ = idx[okc]
        sc = scored[:, okc]
        o["z_pred"][s_] = 0.0
        o["z_pred"][s_, :m] = u.mz[okc]
        o["S"][s_] = 0.0
        o["S"][s_[:, None, None], np.arange(m)[None, :, None], np.arange(m)[None, None, :]] = u.S[okc]
        for k in range(K):
            o["innov"][k][s_, :m] = np.where(sc[k][:, None], nu[k][okc], np.nan)
            o["maha"][k][s_] = np.where(sc[k], d2[k][okc], np.nan)
            o["loglik"][k][s_] = np.where(sc[k], loglik[k][okc], np.nan)
            o["weight_used"][k][s_] = np.where(finite[k][okc], beta[k][okc].astype(np.float64), np.nan)
        o["beta0"][s_] = beta0[okc].astype(np.float64)
        o["innov_comb"][s_, :m] = nub[okc].astype(np.float64)
        n_used[s_] = used.sum(axis=0)[okc]
        wrote = okc & accept
        if commit:
            o["mu"][idx[wrote]], o["cov"][idx[wrote]] = m2[wrote], C2[wrote]
    o["n_used"], o["status"] = n_used, status
    return o


# ---------------------------------------------------------------------------------------------- the end-to-end scenes
E2E_GATE = 16.0
E2E_K = 5
E2E_SIGMA = np.sqrt(0.02)           # about one sigma of S = P_pos + Q for the synthetic initial covariance and E2E_Q
E2E_Q = 0.0097 * np.eye(3)
E2E_SPACING = 1.5                   # sigmas between neighbouring tracks (the assignment's scenes: 6): chosen on the reference alone
E2E_RULE = pr.RULE._replace(clutter_m3=20.0)   # one false detection per 0.05 units of volume: det(2 pi S)^(1/2) is about 0.045 here


def end_to_end_case(mu0, cov0, seed=5, spacing=E2E_SPACING):
    """The assignment test's scenes (assign_reference.end_to_end_case: T = 2, 3, 4 tracks in turn on a line, the scene's
    orientation for every track, K = 5 detections per scene in the world) with the tracks moved together to `spacing` sigmas,
    so that neighbours share detections inside their gates: detection t lies near track t, displaced towards its neighbour, the
    rest is clutter far outside every gate.  One-track scenes fill what is left.  -> dict(mu, cov, Q, starts, z_point [K, n, 3]
    = what POSE_POINT measures of the origin from the detections with the identity mount)."""
    rng = np.random.default_rng(seed)
    n = len(mu0)
    mu, cov = mu0.copy(), cov0.copy()
    scale = np.ones(cov.shape[-1])
    scale[3:6] = 0.1
    cov = cov * scale[:, None] * scale[None, :]
    starts, at, s = [0], 0, 0
    while at + 2 + s % 3 <= n:
        at += 2 + s % 3
        starts.append(at)
        s += 1
    while at < n:
        at += 1
        starts.append(at)
    starts = np.array(starts, dtype=np.int32)
    w = np.empty((E2E_K, n, 3))
    for s in range(len(starts) - 1):
        a, b = starts[s], starts[s + 1]
        T = b - a
        base = rng.uniform(-0.2, 0.2, size=3)
        tracks = base + E2E_SIGMA * spacing * np.arange(T)[:, None] * np.array([1.0, 0.0, 0.0])
        mu[a:b, 0:3] = tracks
        mu[a:b, 3:7] = mu0[a, 3:7]
        det = np.tile(base + np.array([-40.0, 40.0, 0.0]), (E2E_K, 1)) + np.arange(E2E_K)[:, None] * np.array([0.0, 0.0, 3.0])
        for t in range(T):
            towards = 0.6 if t + 1 < T else -0.6
            for _ in range(100):   # drawn again while some track of the scene sees it within 10 % of the gate (S is about sigma^2 I)
                det[t] = tracks[t] + E2E_SIGMA * (np.array([towards, 0.0, 0.0]) + 0.7 * rng.standard_normal(3))
                d2 = ((det[t] - tracks) ** 2).sum(axis=1) / E2E_SIGMA ** 2
                if (np.abs(d2 - E2E_GATE) >= 0.1 * E2E_GATE).all():
                    break
        det = det[rng.permutation(E2E_K)]
        w[:, a:b] = det[:, None, :]
    q = mu[:, 3:7]
    z_point = -on.quat_rotate(on.quat_inverse(q)[None], w)
    return {"mu": mu, "cov": cov, "Q": np.tile(E2E_Q, (n, 1, 1)), "starts": starts, "z_point": z_point}


def reference_chain(man, mu, cov, zs, Q, starts, rule=E2E_RULE, gate=E2E_GATE, dtype=np.float64):
    """update_pda(commit = 0) -> jpda_scenes into its beta, beta0 -> update_weighted, on the state and inputs as stored.
    -> (pda, joint beta [K, n] as the engine stores it, joint beta0, the committed update)"""
    pda = pr.update_pda(man, mu, cov, sr.POSE_POINT, zs, Q, sr.IDENTITY_MOUNT, np.zeros(3), rule=rule, gate_chi2=gate, commit=False)
    st = lambda x: x.astype(dtype).astype(np.float64)   # noqa: E731
    ll, d2 = st(pda["loglik"]), st(pda["maha"])
    j = jpda_scenes(man, ll, d2, starts, sr.POSE_POINT, rule, gate, dtype)
    beta, beta0 = st(pda["beta"]), st(pda["beta0"])
    cov_mask = covered(starts, len(mu))
    beta[:, cov_mask], beta0[cov_mask] = st(j["beta"][:, cov_mask]), st(j["beta0"][cov_mask])
    upd = update_weighted(man, mu, cov, sr.POSE_POINT, zs, Q, sr.IDENTITY_MOUNT, np.zeros(3), beta)
    return pda, beta, beta0, upd, j


def share_of_scenes_that_differ(pda, beta, starts, margin=0.05):
    """among the scenes of two or more tracks: the share in which some pair has |beta_JPDA - beta_PDA| >= margin"""
    hits = total = 0
    for a, b in zip(starts[:-1], starts[1:]):
        if b - a < 2:
            continue
        total += 1
        d = np.abs(np.nan_to_num(beta[:, a:b]) - np.nan_to_num(pda["beta"][:, a:b]))
        hits += bool((d >= margin).any())
    return hits / total
