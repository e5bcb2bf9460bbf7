"""The NumPy reference of the assignment across the filters of a scene (tests/assign_reference.py, include/ukf_batch_assign.h)
against brute force over every matching, against scipy's linear_sum_assignment on the augmented matrix, under permutations, and
on its miss rules; and the conditions the GPU tests (tests/test_gpu_assign.py) rely on, asserted on the very inputs they use:
quantised costs make every objective exact, the product scene's last sweep takes all 32 steps, and every end-to-end scene has
a unique optimum with a margin of 1.0, a quarter of them with a detection that the per-filter choice claims twice."""
import numpy as np
import pytest

import assign_reference as ar
import associate_reference as asr
import sensor_meas_reference as smr
from innovation_reference import reference, reference_scores

CAPACITY = 1022   # of the GPU tests


def random_problem(rng, T, K, forbidden=0.2, quantise=True):
    cost = ar.quantised(rng, (T, K)) if quantise else rng.uniform(0.0, 30.0, size=(T, K))
    cost[rng.random((T, K)) < forbidden] = rng.choice([np.nan, np.inf, 2e100, -np.inf])
    miss = ar.quantised(rng, T) if quantise else rng.uniform(0.0, 30.0, size=T)
    miss[rng.random(T) < 0.1] = np.nan
    gate = float(rng.choice([-1.0, 24.0, 48.0]))
    return cost, miss, gate


def test_against_brute_force_over_all_matchings():
    rng = np.random.default_rng(1)
    for _ in range(300):
        T, K = rng.integers(1, 6, size=2)
        cost, miss, gate = random_problem(rng, T, K, quantise=bool(rng.integers(2)))
        assign, J = ar.solve_scene(cost, miss, gate)
        assert ar.is_valid(cost, miss, gate, assign)
        want = ar.brute_force(cost, miss, gate)
        assert abs(J - want) <= 1e-12 * (1.0 + abs(want)), (cost, miss, gate)
        assert J == ar.objective_of(cost, miss, assign)


def test_against_scipy_on_the_augmented_matrix():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(2)
    for _ in range(400):
        T, K = rng.integers(1, 33, size=2)
        cost, miss, gate = random_problem(rng, T, K)
        A, rows = ar.augmented(cost, miss, gate)
        _, J = ar.solve_scene(cost, miss, gate)
        if len(rows) == 0:
            assert J == 0.0
            continue
        big = np.where(np.isfinite(A), A, 1e9)   # every row has its finite miss column: no forbidden entry is ever chosen
        r, c = opt.linear_sum_assignment(big)
        assert np.isfinite(A[r, c]).all()
        assert J == A[r, c].sum()   # quantised: exact


def test_permuting_tracks_or_detections_permutes_the_answer():
    rng = np.random.default_rng(3)
    for _ in range(100):
        T, K = rng.integers(2, 12, size=2)
        cost = rng.uniform(0.0, 30.0, size=(T, K))   # continuous: the optimum is unique
        miss = np.full(T, 20.0)
        assign, J = ar.solve_scene(cost, miss)
        pt, pk = rng.permutation(T), rng.permutation(K)
        a2, J2 = ar.solve_scene(cost[pt][:, pk], miss[pt])
        assert abs(J2 - J) <= 1e-12 * (1.0 + J)
        back = np.where(a2 >= 0, pk[np.maximum(a2, 0)], -1)
        assert np.array_equal(back, assign[pt])


def test_miss_rules():
    rng = np.random.default_rng(4)
    for _ in range(50):
        T, K = rng.integers(1, 20, size=2)
        cost = ar.quantised(rng, (T, K)) + 1.0
        cost[rng.random((T, K)) < 0.3] = np.inf
        a, J = ar.solve_scene(cost, np.full(T, 0.5))           # a miss below every cost: nobody takes a detection
        assert (a == -1).all() and J == 0.5 * T
        a, _ = ar.solve_scene(cost, np.full(T, 2.0 ** 20))     # a huge miss: maximum cardinality
        opt = pytest.importorskip("scipy.sparse.csgraph")
        from scipy.sparse import csr_matrix
        card = (opt.maximum_bipartite_matching(csr_matrix(np.isfinite(cost)), perm_type="column") >= 0).sum()
        assert (a >= 0).sum() == card
        miss = np.full(T, 20.0)
        out = rng.random(T) < 0.4
        miss[out] = rng.choice([np.nan, np.inf, -np.inf, 2e100], size=out.sum())
        a, J = ar.solve_scene(cost, miss)                      # ineligible tracks: -1, and the others solve without them
        a2, J2 = ar.solve_scene(cost[~out], miss[~out])
        assert (a[out] == -1).all() and np.array_equal(a[~out], a2) and J == J2


def test_second_best_is_the_next_objective():
    rng = np.random.default_rng(6)
    for _ in range(100):
        T, K = rng.integers(1, 4, size=2)
        cost = rng.uniform(0.0, 30.0, size=(T, K))
        miss = np.full(T, 16.0)
        ok = ar.allowed_pairs(cost, 16.0)
        values = []
        import itertools
        for pick in itertools.product(range(-1, K), repeat=T):
            taken = [k for k in pick if k >= 0]
            if len(set(taken)) == len(taken) and all(k < 0 or ok[i, k] for i, k in enumerate(pick)):
                values.append(ar.objective_of(cost, miss, pick))
        values.sort()
        want = values[1] if len(values) > 1 else np.inf
        got = ar.second_best(cost, miss, 16.0)
        assert got == want or abs(got - want) <= 1e-12 * (1.0 + want)


def test_bad_scene_rule_and_uniform_starts():
    assert ar.segment_ok(0, 0, 10) and ar.segment_ok(0, 10, 10) and ar.segment_ok(3, 35, 40)
    assert not ar.segment_ok(-1, 3, 10) and not ar.segment_ok(5, 11, 10) and not ar.segment_ok(5, 4, 10) and not ar.segment_ok(0, 33, 40)
    assert ar.uniform_starts(10, 4).tolist() == [0, 4, 8, 10] and ar.uniform_starts(10, 4, 2).tolist() == [0, 4, 8]
    cost = np.zeros((2, 10))
    out = ar.assign_scenes(cost, np.array([0, 4, 2, 6, 12]), 1.0)
    assert out["scene_status"].tolist() == [0, 1, 0, 1]
    assert (out["assign"][6:] == -7).all() and (out["owner"][1] == -7).all() and out["objective"][3] == -7.0


# ------------------------------------------------------------------------------ what the GPU tests rely on, on their inputs
def test_quantised_costs_make_the_objective_exact():
    """Costs, misses and gates are multiples of 2^-6 in [0, 64): exact in fp32, and every sum and difference the solver forms is
    a multiple of 2^-6 below 2^13, exact in fp64.  So J is the same number whatever optimum is found and in whatever order it
    is summed: 3 000 random ragged, gated problems against scipy, == to the last bit, and the longest sweep within bounds."""
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(7)
    longest = 0
    for _ in range(3000):
        T, K = int(rng.integers(0, 33)), int(rng.integers(1, 33))
        cost, miss, gate = random_problem(rng, T, K)
        assert np.array_equal(ar.stored(cost, np.float32)[np.isfinite(cost) & (np.abs(cost) < 1e30)], cost[np.isfinite(cost) & (np.abs(cost) < 1e30)])
        assign, J, steps = ar.solve_scene(cost, miss, gate, with_steps=True)
        longest = max(longest, steps)
        assert ar.is_valid(cost, miss, gate, assign)
        A, rows = ar.augmented(cost, miss, gate)
        if len(rows):
            r, c = opt.linear_sum_assignment(np.where(np.isfinite(A), A, 1e9))
            assert J == A[r, c].sum()
        else:
            assert J == 0.0
    assert longest <= 64
    for seed, K, per in ((11, 1, False), (12, 5, True), (13, 32, True)):   # the ragged inputs themselves
        cost, miss = ar.ragged_problem(seed, CAPACITY, K, per)
        fin = np.isfinite(cost) & (np.abs(cost) <= ar.COST_MAX)
        assert 0.7 < fin.mean() < 0.9
        assert np.array_equal(cost[fin] / ar.QUANTUM, np.round(cost[fin] / ar.QUANTUM)) and cost[fin].max() < 64.0
        assert np.array_equal(ar.stored(cost, np.float32)[fin], cost[fin]) and not ar.value_ok(ar.stored(cost, np.float32)[~fin]).any()
    starts = ar.ragged_starts(CAPACITY)
    sizes = np.diff(starts)
    assert starts[0] == 6 and starts[-1] == CAPACITY and set(sizes[:-1].tolist()) == set(ar.RAGGED_SIZES)
    # four scenes per workgroup: the scenes of every size fall on every position of a workgroup
    assert all({int(i) % 4 for i in np.nonzero(sizes == t)[0]} == {0, 1, 2, 3} for t in (1, 31, 32))


def test_the_product_scene_takes_all_32_steps():
    cost, miss = ar.product_scene()
    assign, J, steps = ar.solve_scene(cost, miss, with_steps=True)
    assert np.array_equal(assign, np.arange(31, -1, -1)) and steps == 32
    assert J == float(np.sum(np.arange(1, 33) * np.arange(32, 0, -1)))


def test_the_end_to_end_scenes_have_one_clear_optimum(spe, onp):
    """Unique optimum with the second best >= J + 1.0: the project's fp32 score bound 1e-4 (1 + d^2), summed over the 2 T <= 8
    pairs of two matchings at d^2 <= 100, stays below 0.1, so 1.0 is ten times clear.  The per-filter choice claims one
    detection twice in at least a quarter of the scenes, and every cost lies 10 % clear of the gate.  Both flows: position
    measurements (ukfb_innovation_dev) and POSE_POINT (ukfb_associate_sensor_dev); inputs as stored in either precision."""
    mu0, cov0 = spe.synth.pose_initial(CAPACITY)
    c = ar.end_to_end_case(mu0, cov0)
    st = c["starts"]
    assert st[0] == 0 and st[-1] == CAPACITY and np.diff(st).max() == 4
    for dtype in (np.float64, np.float32):
        mu, cov, Q = (ar.stored(c[k], dtype) for k in ("mu", "cov", "Q"))
        m, manz, mz, S, ok, conv = reference(onp, "pose", 0, mu, cov, Q)
        assert ok.all() and conv.all()
        d2_pos = reference_scores(onp, False, m, manz, mz, S, ar.stored(c["z_pos"], dtype))[1]
        r = asr.associate_sensor(onp.POSE, mu, cov, smr.POSE_POINT, ar.stored(c["z_point"], dtype), Q, smr.IDENTITY_MOUNT, np.zeros(3),
                                 gate_chi2=ar.E2E_GATE, commit=False)
        assert (r["status"] == 0).all()
        for d2 in (d2_pos, r["maha"]):
            assert np.isfinite(d2).all() and not ((d2 > 0.9 * ar.E2E_GATE) & (d2 < 1.1 * ar.E2E_GATE)).any()
            best, _ = asr.pick_best(d2, ar.E2E_GATE)
            twice = 0
            for s in range(len(st) - 1):
                a, b = st[s], st[s + 1]
                miss = np.full(b - a, ar.E2E_GATE)
                assign, J = ar.solve_scene(d2[:, a:b].T, miss, ar.E2E_GATE)
                assert ar.second_best(d2[:, a:b].T, miss, ar.E2E_GATE) >= J + 1.0
                assert d2[:, a:b][np.maximum(assign, 0), np.arange(b - a)][assign >= 0].max() <= 100.0
                taken = best[a:b][best[a:b] >= 0]
                twice += len(set(taken.tolist())) != len(taken)
                assert len(set(assign[assign >= 0].tolist())) == (assign >= 0).sum() == b - a   # everybody gets a detection of their own
            assert twice >= (len(st) - 1) / 4
