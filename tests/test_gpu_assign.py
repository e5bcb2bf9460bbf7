"""Assignment across the filters of a scene on the device (ukfb_assign_scenes_dev / ukfb_assign_scenes,
include/ukf_batch_assign.h) against tests/assign_reference.py.

Any optimum is a correct answer, so the comparisons are of two kinds.  On QUANTISED costs (multiples of 2^-6 in [0, 64), exact
in fp32; every sum and difference the solver forms is exact in fp64) the objective must be EQUAL to the reference's, whatever
optimum either found, and the matching must be valid and reproduce that objective from the inputs.  On the end-to-end scenes the
optimum is unique with a margin of 1.0 (asserted on these inputs by tests/test_assign_reference.py), so `assign` itself equals
the reference's.  Capacity 1022: scenes straddle the workgroups of four, the last scene ends at the capacity.
Tolerances of the committed states: those of their families, 1e-9 (fp64) / 1e-4 (fp32): |x - ref| <= tol after
ukfb_update_dev (tests/test_gpu_innovation.py), |x - ref| <= tol (1 + |ref|) after ukfb_update_sensor_dev
(tests/sensor_meas_cases.py)."""
import numpy as np
import pytest
import torch

import assign_reference as ar
import associate_reference as asr
import sensor_meas_reference as smr
from engine_support import new_engine, same_snapshot, scaled, snapshot, tdt
from probe_support import LDS_PATTERNS, lds_poison

pytestmark = pytest.mark.gpu

N = 1022
GUARD = 96
PRECS = [("f64", 0, 1e-9), ("f32", 1, 1e-4)]
I32_SENTINEL, F64_SENTINEL, U32_SENTINEL = -7, -7.0, 0x7FFF


# ---------------------------------------------------------------------------------------------------------------- helpers
_ENGINES = {}


def engine(spe, model, prec):
    """one initialised engine per (model, precision) for the whole module: the call is read-only"""
    if (model, prec) not in _ENGINES:
        e = new_engine(spe, model, N, prec, 0)
        mu, cov = spe.synth.pose_initial(N) if model == "pose" else spe.synth.orient_initial(N)
        e.initialize(mu, cov)
        _ENGINES[model, prec] = e
    return _ENGINES[model, prec]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    while _ENGINES:
        _ENGINES.popitem()[1].close()


def guarded(n, dtype, sentinel):
    """a device buffer of n elements between two guard regions, all of it `sentinel`: (whole, interior view)"""
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def run(e, cost, starts=None, gate=-1.0, miss=0.0, tracks_per_scene=0, scenes=None, want=("assign", "owner", "objective", "scene_status")):
    """cost [K, N] as the engine stores it; starts: offsets or None (uniform mode); miss: a float or an array [N].  Returns the
    outputs as NumPy arrays, and "guards": True while every guard region still holds its sentinel."""
    K = cost.shape[0]
    if scenes is None:
        scenes = len(starts) - 1 if starts is not None else -(-N // tracks_per_scene)
    t = tdt(e)
    with np.errstate(over="ignore"):
        cost_t = torch.from_numpy(np.ascontiguousarray(cost.astype(e.dtype))).cuda()
        miss_t = None if np.isscalar(miss) else torch.from_numpy(np.ascontiguousarray(np.asarray(miss).astype(e.dtype))).cuda()
    assert cost_t.dtype == t
    starts_t = None if starts is None else torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int32)).cuda()
    spec = {"assign": (N, torch.int32, I32_SENTINEL), "owner": (scenes * K, torch.int32, I32_SENTINEL),
            "objective": (scenes, torch.float64, F64_SENTINEL), "scene_status": (scenes, torch.int32, U32_SENTINEL)}
    bufs = {k: guarded(*spec[k]) for k in want}
    torch.cuda.synchronize()
    e.assign_scenes_dev(K, cost_t, scenes, scene_start_dev=starts_t, tracks_per_scene=tracks_per_scene, gate=gate, miss_dev=miss_t,
                        miss=miss if np.isscalar(miss) else 0.0, **{k: v[1] for k, v in bufs.items()})
    e.sync()
    out = {k: v[1].cpu().numpy().copy() for k, v in bufs.items()}
    if "owner" in out:
        out["owner"] = out["owner"].reshape(scenes, K)
    out["guards"] = all(bool((w[:GUARD] == spec[k][2]).all()) and bool((w[GUARD + spec[k][0]:] == spec[k][2]).all()) for k, (w, _) in bufs.items())
    out["_assign_t"] = bufs["assign"][1] if "assign" in bufs else None
    return out


def check_scenes(out, cost, starts, gate, miss, exact_assign=False):
    """every good scene of a launch against the reference on the same (stored) inputs; returns the reference"""
    K = cost.shape[0]
    miss = np.broadcast_to(np.asarray(miss, dtype=np.float64), (N,))
    ref = ar.assign_scenes(cost, starts, miss, gate, sentinel=I32_SENTINEL)
    assert np.array_equal(out["scene_status"], np.where(ref["scene_status"] == ar.BAD_SCENE, ar.BAD_SCENE, ar.OK))
    for s in range(len(starts) - 1):
        a, b = int(starts[s]), int(starts[s + 1])
        if ref["scene_status"][s] == ar.BAD_SCENE:
            continue
        c, m, asg = cost[:, a:b].T, miss[a:b], out["assign"][a:b]
        assert ar.is_valid(c, m, gate, asg), (s, asg)                 # in [-1, K), nothing twice, no forbidden pair, no ineligible track
        assert np.array_equal(out["owner"][s], ar.owner_of(asg, a, K)), s   # owner is the inverse of assign
        J = ar.objective_of(c, m, asg)
        assert J == ref["objective"][s] == out["objective"][s], (s, J, ref["objective"][s], out["objective"][s])
        if exact_assign:
            assert np.array_equal(asg, ref["assign"][a:b]), s
    return ref


def covered(starts):
    mask = np.zeros(N, dtype=bool)
    for a, b in zip(starts[:-1], starts[1:]):
        if ar.segment_ok(int(a), int(b), N):
            mask[a:b] = True
    return mask


# ---------------------------------------------------------------------------------------------------------- 1: ragged scenes
@pytest.mark.parametrize("name,prec,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("K,seed", [(1, 11), (5, 12), (32, 13)])
def test_ragged_scenes(spe, name, prec, tol, K, seed):
    """scene sizes cycling through 0, 1, 2, 3, 5, 8, 16, 31, 32 from slot 6 to the capacity; quantised costs with 20 % of the
    pairs NaN, +inf or beyond 1e100; the gate off and on; miss uniform and per filter with NaN entries"""
    e = engine(spe, "pose", prec)
    starts = ar.ragged_starts(N)
    for per_filter in (False, True):
        cost, miss = ar.ragged_problem(seed + 100 * per_filter, N, K, per_filter)
        cost = ar.stored(cost, e.dtype)
        for gate in (-1.0, 40.0):
            out = run(e, cost, starts, gate=gate, miss=miss if per_filter else 20.0)
            assert out["guards"]
            check_scenes(out, cost, starts, gate, miss)
            assert (out["assign"][:6] == I32_SENTINEL).all() and (out["assign"][6:] != I32_SENTINEL).all()   # the slots before the first scene
            assert ((out["assign"] >= 0).sum() > 0) and ((out["assign"][6:] == -1).sum() > 0)


def test_orientation_engine_plumbing(spe):
    e = engine(spe, "orient", 1)
    starts = ar.ragged_starts(N)
    cost, miss = ar.ragged_problem(21, N, 5, True)
    cost = ar.stored(cost, e.dtype)
    out = run(e, cost, starts, gate=40.0, miss=miss)
    assert out["guards"]
    check_scenes(out, cost, starts, 40.0, miss)


# ------------------------------------------------------------------------------------------------------ 2: structured scenes
@pytest.mark.parametrize("name,prec,tol", PRECS, ids=[p[0] for p in PRECS])
def test_structured_scenes(spe, name, prec, tol):
    e = engine(spe, "pose", prec)
    starts = ar.uniform_starts(N, 32)
    # the product scene in every scene slot of a workgroup: the anti-diagonal, after a last sweep of 32 steps
    pc, pm = ar.product_scene()
    cost = np.zeros((32, N))
    for a, b in zip(starts[:-1], starts[1:]):
        cost[:, a:b] = pc[:b - a].T
    out = run(e, cost, starts, miss=float(pm[0]))
    assert out["guards"]
    check_scenes(out, cost, starts, -1.0, float(pm[0]))
    full = np.diff(starts) == 32
    assert full.sum() >= 8
    for s in np.nonzero(full)[0]:
        assert np.array_equal(out["assign"][starts[s]:starts[s + 1]], np.arange(31, -1, -1)), s
    # all-equal costs: a valid matching, the exact objective, two runs bit-identical
    cost = np.full((32, N), 3.0)
    first = run(e, cost, starts, miss=5.0)
    again = run(e, cost, starts, miss=5.0)
    check_scenes(first, cost, starts, -1.0, 5.0)
    assert all(np.array_equal(first[k], again[k]) for k in ("assign", "owner", "objective", "scene_status"))
    assert (first["assign"] >= 0).all()
    # negative costs, the gate at zero: only the negative pairs are allowed
    rng = np.random.default_rng(31)
    cost = ar.quantised(rng, (7, N)) - 32.0
    for gate in (-1.0, 0.0):
        out = run(e, cost, ar.uniform_starts(N, 5), gate=gate, miss=-3.0)
        check_scenes(out, cost, ar.uniform_starts(N, 5), gate, -3.0)
    # miss below everything: nobody takes a detection; above everything: as many as can
    cost = ar.quantised(rng, (5, N)) + 1.0
    s8 = ar.uniform_starts(N, 8)
    out = run(e, cost, s8, miss=0.5)
    check_scenes(out, cost, s8, -1.0, 0.5)
    assert (out["assign"] == -1).all() and (out["owner"] == -1).all() and np.array_equal(out["objective"], 0.5 * np.diff(s8))
    out = run(e, cost, s8, miss=2.0 ** 20)
    check_scenes(out, cost, s8, -1.0, 2.0 ** 20)
    assert np.array_equal((out["owner"] >= 0).sum(axis=1), np.minimum(np.diff(s8), 5))


# ------------------------------------------------------------------------------------------------------------ 3: bad scenes
@pytest.mark.parametrize("name,prec,tol", PRECS, ids=[p[0] for p in PRECS])
def test_bad_scenes_are_refused_and_touch_nothing(spe, name, prec, tol):
    """Offsets the kernel cannot trust: non-monotone, an end beyond the capacity, a negative start, 33 tracks.  The kernel
    refuses each (no access is made with them: nothing here faults), and the good scenes of the same launch are right."""
    e = engine(spe, "pose", prec)
    #                  good     good      BAD (back)  good       BAD (33)   good        BAD (beyond)  BAD (negative)  good
    starts = np.array([100, 105, 137,     10,         42,        75,        90,         N + 40,       -3,             150, 162], dtype=np.int32)
    rng = np.random.default_rng(41)
    cost = ar.quantised(rng, (6, N))
    out = run(e, cost, starts, gate=48.0, miss=20.0)
    assert out["guards"]
    ref = check_scenes(out, cost, starts, 48.0, 20.0)
    bad = ref["scene_status"] == ar.BAD_SCENE
    assert np.nonzero(bad)[0].tolist() == [2, 4, 6, 7, 8]   # (137, 10), (42, 75), (90, N + 40), (N + 40, -3), (-3, 150)
    assert (out["owner"][bad] == I32_SENTINEL).all() and (out["objective"][bad] == F64_SENTINEL).all()
    assert (out["owner"][~bad] != I32_SENTINEL).all()
    written = covered(starts)
    assert (out["assign"][~written] == I32_SENTINEL).all() and (out["assign"][written] != I32_SENTINEL).all()
    assert not written[42:75].any() and written[10:42].all() and written.sum() == 5 + 32 + 32 + 15 + 12
    # the host-array form knows the offsets and refuses them before any launch
    with pytest.raises(spe.UkfbError, match="code 4"):
        e.assign_scenes(cost, scene_start=starts, gate=48.0, miss=20.0)


# -------------------------------------------------------------------------------------------- 4: uniform mode, host-array form
@pytest.mark.parametrize("name,prec,tol", PRECS, ids=[p[0] for p in PRECS])
def test_uniform_mode_equals_offsets_mode_and_the_host_form(spe, name, prec, tol):
    e = engine(spe, "pose", prec)
    rng = np.random.default_rng(51)
    for T0, K in ((1, 3), (4, 4), (7, 9), (32, 32)):
        cost = ar.stored(ar.ragged_problem(60 + T0, N, K, False)[0], e.dtype)
        miss = ar.quantised(rng, N)
        starts = ar.uniform_starts(N, T0)
        by_offsets = run(e, cost, starts, gate=40.0, miss=miss)
        uniform = run(e, cost, None, gate=40.0, miss=miss, tracks_per_scene=T0)
        assert uniform["guards"] and by_offsets["guards"]
        assert all(np.array_equal(uniform[k], by_offsets[k]) for k in ("assign", "owner", "objective", "scene_status"))
        check_scenes(uniform, cost, starts, 40.0, miss)
        # fewer scenes than fit: the rest is not written
        few = run(e, cost, None, gate=40.0, miss=miss, tracks_per_scene=T0, scenes=3)
        assert np.array_equal(few["assign"][:3 * T0], uniform["assign"][:3 * T0]) and (few["assign"][3 * T0:] == I32_SENTINEL).all()
        assert np.array_equal(few["owner"], uniform["owner"][:3])
        # a single output is enough
        only = run(e, cost, None, gate=40.0, miss=miss, tracks_per_scene=T0, want=("objective",))
        assert np.array_equal(only["objective"], uniform["objective"]) and only["guards"]
    # the host-array form: doubles in, the same answer; slots no scene covers read -1
    cost = ar.stored(ar.ragged_problem(71, N, 5, False)[0], e.dtype)
    starts = ar.ragged_starts(N)
    dev = run(e, cost, starts, gate=40.0, miss=20.0)
    got = e.assign_scenes(cost, scene_start=starts, gate=40.0, miss=20.0)
    assert np.array_equal(got["assign"][6:], dev["assign"][6:]) and (got["assign"][:6] == -1).all()
    assert all(np.array_equal(got[k], dev[k]) for k in ("owner", "objective", "scene_status"))
    got = e.assign_scenes(cost, tracks_per_scene=4, miss=np.full(N, 20.0))
    ref = run(e, cost, None, miss=20.0, tracks_per_scene=4)
    assert all(np.array_equal(got[k], ref[k]) for k in ("assign", "owner", "objective", "scene_status"))
    # argument errors, decided before any launch
    for kw, code in ((dict(tracks_per_scene=0), 4), (dict(tracks_per_scene=33), 4), (dict(tracks_per_scene=4, scenes=257), 4),
                     (dict(tracks_per_scene=4, scenes=-1), 4), (dict(tracks_per_scene=4, miss=float("nan")), 1)):
        with pytest.raises(spe.UkfbError, match=f"code {code}"):
            e.assign_scenes(cost, **kw)
    with pytest.raises(spe.UkfbError, match="code 1"):
        e.assign_scenes_dev(5, dev["_assign_t"], 3, tracks_per_scene=4)   # every output NULL


# ------------------------------------------------------------------------------------------------------------ 5, 6: end to end
def e2e_engine(spe, prec):
    mu0, cov0 = spe.synth.pose_initial(N)
    c = ar.end_to_end_case(mu0, cov0)
    e = spe.BatchPoseUKF(N, precision=prec, gate_chi2=ar.E2E_GATE)
    e.initialize(c["mu"], c["cov"])
    mu, cov, _ = e.state()
    return e, c, mu, cov


def reference_choice(c, d2):
    """the reference's assignment of the constructed scenes from reference scores, and the per-filter nearest gated candidate"""
    ref = ar.assign_scenes(d2, c["starts"], ar.E2E_GATE, ar.E2E_GATE)
    return ref, asr.pick_best(d2, ar.E2E_GATE)[0]


def has_duplicates(c, pick):
    st = c["starts"]
    return np.array([len(set(p[p >= 0].tolist())) != (p >= 0).sum() for p in (pick[a:b] for a, b in zip(st[:-1], st[1:]))])


@pytest.mark.parametrize("name,prec,tol", PRECS, ids=[p[0] for p in PRECS])
def test_state_selecting_end_to_end(spe, onp, name, prec, tol):
    """ukfb_innovation_dev -> assign (miss = gate) -> ukfb_select_candidates_dev -> ukfb_update_dev on the constructed scenes"""
    from innovation_reference import reference, reference_scores
    e, c, mu, cov = e2e_engine(spe, prec)
    t, K = tdt(e), ar.E2E_K
    Qs, zs = ar.stored(c["Q"], e.dtype), ar.stored(c["z_pos"], e.dtype)
    m, manz, mz, S, ok, conv = reference(onp, "pose", 0, mu, cov, Qs)
    d2 = reference_scores(onp, False, m, manz, mz, S, zs)[1]
    ref, ref_best = reference_choice(c, d2)
    z_t = torch.from_numpy(np.ascontiguousarray(c["z_pos"])).to("cuda", t)
    Q_t = torch.from_numpy(np.ascontiguousarray(c["Q"]).reshape(-1)).to("cuda", t)
    maha = torch.full((K, N), 7.0, dtype=t, device="cuda")
    best = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    assign = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    starts_t = torch.from_numpy(c["starts"]).cuda()
    z_sel = torch.full((N, 3), 9.0, dtype=t, device="cuda")
    m_sel = torch.full((N,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.innovation_dev(0, K, z_t, Q_t, maha=maha, best=best)
    e.assign_scenes_dev(K, maha, len(c["starts"]) - 1, scene_start_dev=starts_t, gate=ar.E2E_GATE, miss=ar.E2E_GATE, assign=assign)
    e.select_candidates_dev(K, assign, 0, z_t, z_sel, m_sel)
    e.update_dev(0, z_sel, Q_t, meas_model_dev=m_sel)
    e.sync()
    got, best = assign.cpu().numpy(), best.cpu().numpy()
    assert np.array_equal(best, ref_best)
    assert np.array_equal(got, ref["assign"]) and (got >= 0).all()
    dup_best, dup_got = has_duplicates(c, best), has_duplicates(c, got)
    assert dup_best.sum() >= len(dup_best) / 4 and not dup_got.any()
    assert (e.status() == 0).all() and (m_sel.cpu().numpy() == 0).all()
    mu2, cov2, _ = e.state()
    m_o, c_o, st_o = onp.pose_update(mu, cov, 0, zs[got, np.arange(N)], Qs)
    assert (st_o == 0).all()
    em, ec = np.abs(mu2 - m_o).max(), np.abs(cov2 - c_o).max()
    print(f"assignment end to end (state) {name}: max|dmu|={em:.3e} max|dcov|={ec:.3e} scenes with a doubly claimed detection={dup_best.sum()}")
    assert em <= tol and ec <= tol
    e.close()


@pytest.mark.parametrize("name,prec,tol", PRECS, ids=[p[0] for p in PRECS])
def test_sensor_frame_end_to_end(spe, onp, name, prec, tol):
    """ukfb_associate_sensor_dev(POSE_POINT, commit = 0) -> assign -> ukfb_select_candidates_dev (the sensor ids pass through
    its per-filter model array) -> ukfb_update_sensor_dev with the per-filter ids"""
    e, c, mu, cov = e2e_engine(spe, prec)
    t, K = tdt(e), ar.E2E_K
    Qs, zs = ar.stored(c["Q"], e.dtype), ar.stored(c["z_point"], e.dtype)
    scores = asr.associate_sensor(onp.POSE, mu, cov, smr.POSE_POINT, zs, Qs, smr.IDENTITY_MOUNT, np.zeros(3), gate_chi2=ar.E2E_GATE, commit=False)
    ref, ref_best = reference_choice(c, scores["maha"])
    z_t = torch.from_numpy(np.ascontiguousarray(c["z_point"])).to("cuda", t)
    Q_t = torch.from_numpy(np.ascontiguousarray(c["Q"]).reshape(-1)).to("cuda", t)
    maha = torch.full((K, N), 7.0, dtype=t, device="cuda")
    best = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    assign = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    starts_t = torch.from_numpy(c["starts"]).cuda()
    ids = torch.full((N,), smr.POSE_POINT, dtype=torch.int32, device="cuda")
    z_sel = torch.full((N, 3), 9.0, dtype=t, device="cuda")
    m_sel = torch.full((N,), 77, dtype=torch.int32, device="cuda")
    before = snapshot(e, noise_of=(0,))
    torch.cuda.synchronize()
    e.associate_sensor_dev(smr.POSE_POINT, K, z_t, Q_t, commit=False, maha=maha, best=best)
    e.assign_scenes_dev(K, maha, len(c["starts"]) - 1, scene_start_dev=starts_t, gate=ar.E2E_GATE, miss=ar.E2E_GATE, assign=assign)
    e.select_candidates_dev(K, assign, 0, z_t, z_sel, m_sel, meas_model_dev=ids)
    e.sync()
    assert same_snapshot(before, snapshot(e, noise_of=(0,)))   # nothing so far has touched the filters
    e.update_sensor_dev(0, z_sel, Q_t, model_dev=m_sel)
    e.sync()
    got, best = assign.cpu().numpy(), best.cpu().numpy()
    assert np.array_equal(best, ref_best)
    assert np.array_equal(got, ref["assign"]) and (got >= 0).all()
    dup_best = has_duplicates(c, best)
    assert dup_best.sum() >= len(dup_best) / 4 and not has_duplicates(c, got).any()
    assert (m_sel.cpu().numpy() == smr.POSE_POINT).all() and (e.status() == 0).all()
    mu2, cov2, _ = e.state()
    want = smr.update_sensor(onp.POSE, mu, cov, smr.POSE_POINT, zs[got, np.arange(N)], Qs, smr.IDENTITY_MOUNT, np.zeros(3))
    assert (want["status"] == 0).all()
    em, ec = scaled(mu2, want["mu"]), scaled(cov2, want["cov"])
    print(f"assignment end to end (sensor frame) {name}: max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e}")
    assert em <= tol and ec <= tol
    e.close()


# ------------------------------------------------------------------------------------------- 7: read-only, leftovers in LDS
@pytest.mark.parametrize("name,prec,tol", PRECS, ids=[p[0] for p in PRECS])
def test_read_only_and_independent_of_lds_leftovers(spe, name, prec, tol):
    e = engine(spe, "pose", prec)
    starts = ar.ragged_starts(N)
    cost, miss = ar.ragged_problem(81, N, 32, True)
    cost = ar.stored(cost, e.dtype)
    before = snapshot(e, noise_of=(0, N - 1))
    clean = run(e, cost, starts, gate=40.0, miss=miss)
    assert same_snapshot(before, snapshot(e, noise_of=(0, N - 1)))
    check_scenes(clean, cost, starts, 40.0, miss)
    poison = lds_poison()
    for pattern in (LDS_PATTERNS[0], LDS_PATTERNS[2]):   # a float NaN; all ones: a NaN in both precisions, -1 as an index
        assert poison(pattern) == 0
        out = run(e, cost, starts, gate=40.0, miss=miss)
        assert all(np.array_equal(out[k], clean[k]) for k in ("assign", "owner", "objective", "scene_status")), hex(pattern)
