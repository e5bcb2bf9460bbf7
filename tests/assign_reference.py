"""NumPy float64 statement of the assignment across the filters of a scene (include/ukf_batch_assign.h): the rules of a pair and of
a track, the shortest augmenting path solver (Jonker-Volgenant for rectangular problems, Crouse 2016) on the T x (K + T) problem
with one private miss column per track, the launch over scenes with the bad-scene rule, the objective recomputed from the
inputs, the second-best optimum, a brute force over every matching, and the inputs the GPU tests use (quantised costs, the product
scene, the end-to-end scenes).  No tests here."""
import itertools

import numpy as np

COST_MAX = 1e100
MAX_TRACKS = 32
MAX_CANDIDATES = 32
OK, BAD_SCENE = 0, 1
INF = np.inf


def value_ok(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (np.abs(v) <= COST_MAX)


def allowed_pairs(cost, gate):
    """cost [T, K] -> bool [T, K]"""
    cost = np.asarray(cost, dtype=np.float64)
    ok = value_ok(cost)
    if gate >= 0:
        with np.errstate(invalid="ignore"):
            ok &= cost <= gate
    return ok


def augmented(cost, miss, gate):
    """The T' x (K + T') matrix of the eligible tracks (in their order), +inf where forbidden, and the eligible tracks' indices."""
    cost = np.asarray(cost, dtype=np.float64)
    miss = np.asarray(miss, dtype=np.float64)
    assert cost.ndim == 2 and cost.shape[0] == len(miss)
    rows = np.nonzero(value_ok(miss))[0]
    T, K = len(rows), cost.shape[1]
    A = np.full((T, K + T), INF)
    c = cost[rows]
    A[:, :K] = np.where(allowed_pairs(c, gate), c, INF)
    A[np.arange(T), K + np.arange(T)] = miss[rows]
    return A, rows


def lapjv(A):
    """Shortest augmenting paths on A [nr, nc], nr <= nc, +inf = forbidden, every row with an allowed column of its own.
    Returns col4row [nr] and the longest sweep's steps.  Ties go to the lowest column."""
    nr, nc = A.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    longest = 0
    for cur in range(nr):
        shortest = np.full(nc, INF)
        path = np.full(nc, -1)
        scanned = np.zeros(nc, dtype=bool)
        i, minv, sink, steps = cur, 0.0, -1, 0
        while sink < 0:
            steps += 1
            assert steps <= nc
            r = minv + A[i] - u[i] - v
            better = ~scanned & (r < shortest)
            shortest[better] = r[better]
            path[better] = i
            key = np.where(scanned, INF, shortest)
            j = int(np.argmin(key))   # the first of equal minima
            assert key[j] < INF
            minv = key[j]
            scanned[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
        longest = max(longest, steps)
        u[cur] += minv
        for i in range(nr):
            if i != cur and col4row[i] >= 0 and scanned[col4row[i]]:
                u[i] += minv - shortest[col4row[i]]
        v[scanned] -= minv - shortest[scanned]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return col4row, longest


def solve_scene(cost, miss, gate=-1.0, with_steps=False):
    """cost [T, K], miss [T] -> (assign [T] with -1 for none, objective)"""
    cost = np.asarray(cost, dtype=np.float64)
    miss = np.asarray(miss, dtype=np.float64)
    T, K = cost.shape
    A, rows = augmented(cost, miss, gate)
    assign = np.full(T, -1, dtype=np.int32)
    steps = 0
    if len(rows):
        col, steps = lapjv(A)
        assign[rows] = np.where(col < K, col, -1)
    J = objective_of(cost, miss, assign)
    return (assign, J, steps) if with_steps else (assign, J)


def objective_of(cost, miss, assign):
    """J recomputed from the inputs: the assigned pairs' costs and the misses of the eligible tracks without a detection"""
    cost = np.asarray(cost, dtype=np.float64)
    miss = np.asarray(miss, dtype=np.float64)
    J = 0.0
    for i, k in enumerate(assign):
        if k >= 0:
            J += cost[i, k]
        elif value_ok(miss[i]):
            J += miss[i]
    return float(J)


def is_valid(cost, miss, gate, assign):
    """in range, no detection twice, no forbidden pair, no ineligible track"""
    cost = np.asarray(cost, dtype=np.float64)
    T, K = cost.shape
    assign = np.asarray(assign)
    if not ((assign >= -1) & (assign < K)).all():
        return False
    taken = assign[assign >= 0]
    if len(set(taken.tolist())) != len(taken):
        return False
    ok, elig = allowed_pairs(cost, gate), value_ok(miss)
    return all(k < 0 or (ok[i, k] and elig[i]) for i, k in enumerate(assign))


def owner_of(assign, first, K):
    """the inverse of a scene's assign: the engine slot that took detection k, or -1"""
    owner = np.full(K, -1, dtype=np.int32)
    for i, k in enumerate(assign):
        if k >= 0:
            owner[k] = first + i
    return owner


def brute_force(cost, miss, gate=-1.0):
    """the optimum over every matching (T, K small)"""
    cost = np.asarray(cost, dtype=np.float64)
    T, K = cost.shape
    ok, elig = allowed_pairs(cost, gate), value_ok(miss)
    best = INF
    for pick in itertools.product(range(-1, K), repeat=T):
        taken = [k for k in pick if k >= 0]
        if len(set(taken)) != len(taken):
            continue
        if any(k >= 0 and not (ok[i, k] and elig[i]) for i, k in enumerate(pick)):
            continue
        best = min(best, objective_of(cost, miss, pick))
    return best


def second_best(cost, miss, gate=-1.0):
    """The best objective among the matchings that differ from the optimum found: the optimum with each of its pairs, and each
    of its misses, forbidden in turn (any other matching lacks at least one of them).  +inf when there is no other matching."""
    cost = np.asarray(cost, dtype=np.float64)
    miss = np.asarray(miss, dtype=np.float64)
    assign, _ = solve_scene(cost, miss, gate)
    A, rows = augmented(cost, miss, gate)
    K = cost.shape[1]
    best = INF
    for r, i in enumerate(rows):
        col = assign[i] if assign[i] >= 0 else K + r
        B = A.copy()
        B[r, col] = INF
        if not np.isfinite(B[r]).any():
            continue   # the track has nothing else to take
        c4r, _ = lapjv(B)
        best = min(best, float(B[np.arange(len(rows)), c4r].sum()))
    return best


def uniform_starts(capacity, tracks_per_scene, scenes=None):
    n = -(-capacity // tracks_per_scene) if scenes is None else scenes
    return np.minimum(np.arange(n + 1, dtype=np.int64) * tracks_per_scene, capacity).astype(np.int32)


def segment_ok(a, b, capacity):
    return a >= 0 and b <= capacity and b >= a and b - a <= MAX_TRACKS


def assign_scenes(cost, scene_start, miss, gate=-1.0, sentinel=-7):
    """The launch: cost [K, capacity], scene_start [scenes + 1], miss [capacity].  Returns a dict: assign [capacity] (`sentinel`
    where nothing is written), owner [scenes, K], objective [scenes] (sentinel on a bad scene), scene_status [scenes]."""
    cost = np.asarray(cost, dtype=np.float64)
    K, cap = cost.shape
    miss = np.broadcast_to(np.asarray(miss, dtype=np.float64), (cap,))
    scenes = len(scene_start) - 1
    out = {"assign": np.full(cap, sentinel, dtype=np.int32), "owner": np.full((scenes, K), sentinel, dtype=np.int32),
           "objective": np.full(scenes, float(sentinel)), "scene_status": np.zeros(scenes, dtype=np.uint32)}
    for s in range(scenes):
        a, b = int(scene_start[s]), int(scene_start[s + 1])
        if not segment_ok(a, b, cap):
            out["scene_status"][s] = BAD_SCENE
            continue
        asg, J = solve_scene(cost[:, a:b].T, miss[a:b], gate)
        out["assign"][a:b] = asg
        out["owner"][s] = owner_of(asg, a, K)
        out["objective"][s] = J
    return out


# ------------------------------------------------------------------------------------------------- the inputs of the GPU tests
QUANTUM = 2.0 ** -6   # costs, misses and gates are multiples of it in [0, 64): exact in fp32, every sum and difference exact in fp64
RAGGED_SIZES = (0, 1, 2, 3, 5, 8, 16, 31, 32)


def quantised(rng, shape):
    return rng.integers(0, 64 * 64, size=shape).astype(np.float64) * QUANTUM


def ragged_starts(capacity, first=6):
    """Scene sizes cycling through RAGGED_SIZES from slot `first`; the last scene ends at capacity."""
    starts, at, i = [first], first, 0
    while at < capacity:
        at = min(at + RAGGED_SIZES[i % len(RAGGED_SIZES)], capacity)
        starts.append(at)
        i += 1
    return np.array(starts, dtype=np.int32)


def ragged_problem(seed, capacity, K, per_filter_miss):
    """Quantised costs with 20 % of the pairs NaN, +inf or beyond COST_MAX on either side (an fp32 engine stores those as
    +-inf: see stored()); miss uniform or per filter with some entries NaN"""
    rng = np.random.default_rng(seed)
    cost = quantised(rng, (K, capacity))
    bad = rng.random((K, capacity))
    cost[bad < 0.07] = np.nan
    cost[(bad >= 0.07) & (bad < 0.14)] = np.inf
    cost[(bad >= 0.14) & (bad < 0.17)] = 2e100
    cost[(bad >= 0.17) & (bad < 0.20)] = -2e100
    if per_filter_miss:
        miss = quantised(rng, capacity)
        miss[rng.random(capacity) < 0.1] = np.nan
    else:
        miss = np.full(capacity, 20.0)
    return cost, miss


def stored(x, dtype):
    """x as an engine of that dtype holds it, in double (values beyond fp32's range become +-inf)"""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)


def product_scene():
    """cost = outer(1 ... 32, 1 ... 32) with a huge miss: the optimum is the anti-diagonal and the last sweep takes all 32 steps"""
    x = np.arange(1.0, 33.0)
    return np.outer(x, x), np.full(32, 2.0 ** 20)


E2E_GATE = 16.0                     # the gate of the end-to-end flows, also their miss: classical global nearest neighbour
E2E_K = 5
E2E_SIGMA = np.sqrt(0.02)           # about one sigma of S = P_pos + Q for the synthetic initial covariance and E2E_Q
E2E_Q = 0.0097 * np.eye(3)
_CONFLICT = ((2.6, 0.0, 0.0), (0.0, 3.6, 0.0))   # detections 0 and 1 of a conflict scene, from tracks 0 and 1, in sigmas
_OWN = ((0.7, 0.0, 2.0), (0.9, 0.5, -0.6))       # a track's own detection: in a conflict scene (tracks >= 2), in a plain scene


def end_to_end_case(mu0, cov0, seed=5):
    """The constructed scenes of the end-to-end tests on `capacity` Pose filters (mu0, cov0: the synthetic initial state).
    Scenes of T = 2, 3, 4 tracks in turn, 6 sigma apart on a line, every track of a scene with the scene's orientation, the
    orientation covariance scaled down by 100 so that S is the position's; K = 5 detections per scene, positions in the world:
    even scenes are CONFLICT scenes: detection 0 lies between tracks 0 and 1 and is the nearest of both (d^2 about 6.8 and
    11.6), detection 1 is track 1's alternative (13.0); the other tracks have a detection of their own, the rest is clutter far
    outside every gate.  Returns dict(mu, cov, Q [n, 3, 3], starts, w [K, n, 3] the detections' world positions per slot,
    z_pos = w, z_point [K, n, 3] = what POSE_POINT measures of the origin from w with the identity mount: -R^T w)."""
    from oracle import ukf_numpy as on
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
    starts = np.array(starts, dtype=np.int32)
    w = np.empty((E2E_K, n, 3))
    w[:] = (-40.0, 40.0, 0.0)
    for s in range(len(starts) - 1):
        a, b = starts[s], starts[s + 1]
        T = b - a
        base = rng.uniform(-0.2, 0.2, size=3)
        tracks = base + E2E_SIGMA * 6.0 * np.arange(T)[:, None] * np.array([1.0, 0.0, 0.0])
        mu[a:b, 0:3] = tracks
        mu[a:b, 3:7] = mu0[a, 3:7]
        det = np.tile(base + np.array([-40.0, 40.0, 0.0]), (E2E_K, 1)) + np.arange(E2E_K)[:, None] * np.array([0.0, 0.0, 3.0])
        jitter = QUANTUM * rng.integers(-2, 3, size=(T, 3))
        for t in range(T):
            if s % 2 == 0:
                off = _CONFLICT[t] if t < 2 else _OWN[0]
            else:
                off = _OWN[1]
            det[t] = tracks[t] + E2E_SIGMA * (np.array(off) + jitter[t])
        det = det[rng.permutation(E2E_K)]   # the detections' order carries no information
        w[:, a:b] = det[:, None, :]
    q = mu[:, 3:7]
    z_point = -on.quat_rotate(on.quat_inverse(q)[None], w)
    return {"mu": mu, "cov": cov, "Q": np.tile(E2E_Q, (n, 1, 1)), "starts": starts, "w": w, "z_pos": w, "z_point": z_point}
