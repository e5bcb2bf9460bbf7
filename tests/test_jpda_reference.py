"""tests/jpda_reference.py held to the definition, and the conditions the GPU tests rely on asserted on their own inputs, on
the CPU: the subset recurrences against brute force over every joint event, their invariances and sums, T = 1 against the
per-filter PDA weights, update_weighted against update_pda, its normalisation and all-zero rules, the stage-typed evaluation
(tests/jpda_f32.py) against it, and the end-to-end scenes' power to tell joint weights from per-filter ones."""
import numpy as np
import pytest

import jpda_f32
import jpda_reference as jr
import pda_reference as pr
import sensor_meas_cases as smc
import sensor_meas_reference as sr
from engine_support import man_of
from oracle import ukf_numpy as on

CAPACITY = 1022
N = 140


def random_scene(rng, T, K, forbid=0.3):
    loglik = -0.5 * rng.uniform(0.0, 20.0, size=(T, K)) - rng.uniform(-1.0, 7.0, size=(T, K))
    loglik[rng.random((T, K)) < forbid] = np.nan
    a0, ln_pd = pr.log_terms(pr.RULE, rng.choice([1, 3], size=T))
    return jr.psi_of(loglik, None, -1.0, a0, ln_pd)


def test_marginals_equal_brute_force_over_every_joint_event():
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(300):
        T, K = int(rng.integers(1, 5)), int(rng.integers(1, 6))
        psi, allowed, _ = random_scene(rng, T, K)
        beta, beta0, Z = jr.marginals(psi)
        b2, b02, Z2 = jr.brute_force(psi)
        worst = max(worst, np.abs(beta - b2).max(), np.abs(beta0 - b02).max(), abs(Z - Z2) / Z2)
        assert (beta[~allowed] == 0.0).all()
    print(f"JPDA-REFERENCE recurrences against brute force, 300 scenes with T <= 4, K <= 5: worst deviation {worst:.2e}")
    assert worst <= 1e-13
    # six tracks once, against brute force (at most 6^6 events here)
    psi, _, _ = random_scene(rng, 6, 5, forbid=0.4)
    beta, beta0, Z = jr.marginals(psi)
    b2, b02, Z2 = jr.brute_force(psi)
    assert np.abs(beta - b2).max() <= 1e-13 and np.abs(beta0 - b02).max() <= 1e-13 and abs(Z - Z2) <= 1e-13 * Z2


def test_permuting_tracks_and_detections_permutes_the_marginals_and_the_sums_hold():
    rng = np.random.default_rng(2)
    for _ in range(100):
        T, K = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        psi, _, _ = random_scene(rng, T, K)
        beta, beta0, Z = jr.marginals(psi)
        pt, pk = rng.permutation(T), rng.permutation(K)
        b2, b02, Z2 = jr.marginals(psi[pt][:, pk])
        assert np.abs(b2 - beta[pt][:, pk]).max() <= 1e-13 and np.abs(b02 - beta0[pt]).max() <= 1e-13 and abs(Z2 - Z) <= 1e-13 * Z
        assert np.abs(beta.sum(axis=1) + beta0 - 1.0).max() <= 1e-13
        assert (beta.sum(axis=0) <= 1.0 + 1e-13).all() and (beta >= 0.0).all() and Z >= 1.0
    # a track with no allowed pair: beta_i0 = 1, and its neighbours' marginals are those of the scene without it
    psi, _, _ = random_scene(rng, 4, 5)
    psi[2] = 0.0
    beta, beta0, _ = jr.marginals(psi)
    rest, rest0, _ = jr.marginals(psi[[0, 1, 3]])
    assert abs(beta0[2] - 1.0) <= 1e-15 and (beta[2] == 0.0).all()
    assert np.abs(beta[[0, 1, 3]] - rest).max() <= 1e-14 and np.abs(beta0[[0, 1, 3]] - rest0).max() <= 1e-14


def test_one_track_scenes_are_the_per_filter_weights():
    rng = np.random.default_rng(3)
    K, B = 5, 200
    loglik, maha = jr.synthetic_scores(31, B, K, np.float64)
    m = rng.choice([1, 3], size=B)
    a0, ln_pd = pr.log_terms(pr.RULE, m)
    for gate in (-1.0, jr.SYNTH_GATE):
        inside = np.isfinite(loglik) & ((gate < 0) | (np.nan_to_num(maha, nan=np.inf) <= gate))
        want, want0 = pr.weights(loglik, inside, a0, ln_pd)
        for i in range(B):
            psi, allowed, _ = jr.psi_of(loglik[:, i][None], maha[:, i][None], gate, a0[i:i + 1], ln_pd)
            assert np.array_equal(allowed[0], inside[:, i])
            beta, beta0, _ = jr.marginals(psi)
            assert np.abs(beta[0] - want[:, i]).max() <= 1e-13 and abs(beta0[0] - want0[i]) <= 1e-13


def test_the_launch_rules():
    assert jr.segment_status(0, 0, 10) == jr.OK and jr.segment_status(0, 6, 10) == jr.OK and jr.segment_status(4, 10, 10) == jr.OK
    assert jr.segment_status(0, 7, 10) == jr.TOO_LARGE and jr.segment_status(3, 35, 40) == jr.TOO_LARGE
    assert all(jr.segment_status(a, b, 40) == jr.BAD_SCENE for a, b in ((-1, 3), (38, 41), (5, 4), (0, 33)))
    assert (jr.MAX_TRACKS, jr.LOG_RATIO_MAX, jr.OK, jr.BAD_SCENE, jr.TOO_LARGE, jr.MAX_CANDIDATES) == (6, 100.0, 0, 1, 2, 32)
    starts = jr.ragged_starts(CAPACITY)
    assert starts[0] == 5 and starts[-1] == CAPACITY and set(np.diff(starts)[:-1].tolist()) == set(range(7))
    # the cap: every l at or above it gives exp(100), and six tracks by 32 detections of them stay finite
    psi, _, _ = jr.psi_of(np.full((6, 32), 500.0), None, -1.0, np.zeros(6), 0.0)
    assert (psi == np.exp(100.0)).all()
    beta, beta0, Z = jr.marginals(psi)
    assert np.isfinite(Z) and np.isfinite(beta).all() and np.abs(beta.sum(axis=1) + beta0 - 1.0).max() <= 1e-12
    # patterns: NaN where loglik is not finite, 0 where it is finite and the gate forbids
    man = man_of("pose")
    ll, d2 = jr.synthetic_scores(5, 30, 4, np.float64)
    o = jr.jpda_scenes(man, ll, d2, np.array([0, 3, 3, 9, 20, 30]), jr.mixed_models(man, 30), gate=jr.SYNTH_GATE)
    assert o["scene_status"].tolist() == [0, 0, 0, 2, 2]
    assert (o["beta"][:, 9:] == -7.0).all() and (o["beta0"][9:] == -7.0).all() and (o["free"][3:] == -7.0).all()
    head = o["beta"][:, :9]
    assert np.array_equal(np.isnan(head), ~np.isfinite(ll[:, :9]))
    forbidden = np.isfinite(ll[:, :9]) & ~(np.nan_to_num(d2[:, :9], nan=np.inf) <= jr.SYNTH_GATE)
    assert (head[forbidden] == 0.0).all() and forbidden.any() and (head[np.isfinite(ll[:, :9]) & ~forbidden] > 0.0).all()


def test_the_synthetic_scores_stay_below_the_cap():
    """the condition of tests/test_gpu_jpda.py: every |l| of its random inputs is below 100, in both precisions"""
    for model in ("pose", "orient"):
        man = man_of(model)
        for dtype in (np.float64, np.float32):
            for K, seed in ((1, 11), (5, 12), (32, 13)):
                ll, _ = jr.synthetic_scores(seed, CAPACITY, K, dtype)
                top = jr.largest_log_ratio(ll, jr.mixed_models(man, CAPACITY), man, pr.RULE, dtype)
                assert top < jr.LOG_RATIO_MAX, top


# ------------------------------------------------------------------------------------------------------- update_weighted
_BATCH = {}


def batch(model, n=N):
    if (model, n) not in _BATCH:
        mu, cov, _ = smc.states(model)
        mu, cov = mu[:n].copy(), cov[:n].copy()
        mount, point, gyro, z, Q = smc.make_inputs(model, mu, np.float64)
        ids = smc.cycling_ids(model, n)
        zt = np.zeros((n, 3))
        for mid in sr.ids_of(man_of(model)):
            zt[ids == mid] = z[mid][ids == mid]
        zs, _ = pr.constructed_pda(man_of(model), mu, cov, ids, zt, Q, mount, point, gyro, 4)
        _BATCH[(model, n)] = (man_of(model), mu, cov, mount, point, gyro, Q, ids, zs)
    return _BATCH[(model, n)]


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and bool((np.abs(a - b)[~np.isnan(b)] <= tol * (1.0 + np.abs(b[~np.isnan(b)]))).all())


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_update_weighted_with_pdas_own_weights_is_update_pda(model):
    man, mu, cov, mount, point, gyro, Q, ids, zs = batch(model)
    pda = pr.update_pda(man, mu, cov, ids, zs, Q, mount, point, gyro, gate_chi2=pr.GATE)
    pr.conditions(pda)
    got = jr.update_weighted(man, mu, cov, ids, zs, Q, mount, point, pda["beta"], gyro)
    assert np.array_equal(got["status"], pda["status"]) and np.array_equal(got["n_used"], pda["n_gated"])
    for k in ("mu", "cov", "z_pred", "S", "innov", "maha", "loglik", "beta0", "innov_comb"):
        assert close(got[k], pda[k]), k
    assert close(got["weight_used"], pda["beta"])
    assert not np.array_equal(got["mu"], mu)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_the_normalisation_rule_and_the_all_zero_rule(model):
    man, mu, cov, mount, point, gyro, Q, ids, zs = batch(model)
    rng = np.random.default_rng(7)
    live = np.isin(ids, sr.ids_of(man))
    w = rng.uniform(0.05, 0.2, size=zs.shape[:2])
    base = jr.update_weighted(man, mu, cov, ids, zs, Q, mount, point, w, gyro)
    s = w.sum(axis=0)
    assert (s < 1.0).all() and close(base["beta0"][live], 1.0 - s[live]) and close(base["weight_used"][:, live], w[:, live])
    # above one: used as w / s, beta_0 = 0, and the state of the weights already normalised
    big = jr.update_weighted(man, mu, cov, ids, zs, Q, mount, point, 3.0 * w / s, gyro)
    unit = jr.update_weighted(man, mu, cov, ids, zs, Q, mount, point, w / s, gyro)
    assert (np.abs(big["beta0"][live]) <= 1e-15).all() and close(big["weight_used"], unit["weight_used"])
    assert close(big["mu"], unit["mu"]) and close(big["cov"], unit["cov"]) and close(big["innov_comb"], unit["innov_comb"])
    # NaN, negative and zero entries do not count; n_used says how many did
    odd = w.copy()
    odd[0], odd[1], odd[2] = np.nan, -0.3, 0.0
    got = jr.update_weighted(man, mu, cov, ids, zs, Q, mount, point, odd, gyro)
    only = np.zeros_like(w)
    only[3] = w[3]
    want = jr.update_weighted(man, mu, cov, ids, zs, Q, mount, point, only, gyro)
    assert (got["n_used"][live] == 1).all() and all(np.array_equal(got[k], want[k], equal_nan=True) for k in got)
    assert (got["weight_used"][:3, live] == 0.0).all()
    # all zero: the state kept bit for bit, REJECTED_GATE, beta_0 = 1
    none = jr.update_weighted(man, mu, cov, ids, zs, Q, mount, point, np.zeros_like(w), gyro)
    assert np.array_equal(none["mu"], mu) and np.array_equal(none["cov"], cov)
    assert (none["status"][live] == on.ST_REJECTED_GATE).all() and (none["beta0"][live] == 1.0).all()
    assert (none["innov_comb"][live] == 0.0).all() and (none["n_used"] == 0).all() and np.isfinite(none["maha"][:, live]).all()
    # commit = 0
    dry = jr.update_weighted(man, mu, cov, ids, zs, Q, mount, point, w, gyro, commit=False)
    assert np.array_equal(dry["mu"], mu) and np.array_equal(dry["beta0"], base["beta0"], equal_nan=True)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_the_stage_typed_evaluation_in_float64_is_the_reference(model):
    man, mu, cov, mount, point, gyro, Q, ids, zs = batch(model)
    w = np.random.default_rng(8).uniform(0.05, 0.4, size=zs.shape[:2])
    ref = jr.update_weighted(man, mu, cov, ids, zs, Q, mount, point, w, gyro)
    used = np.nan_to_num(ref["weight_used"], nan=0.0) > 0.0
    keep = (ref["n_used"] == 0) | (ref["status"] != 0)
    o = {p: jpda_f32.weighted(model, mu, cov, ids, zs, Q, mount, point, gyro, w, used, keep=keep, prec=p) for p in ("f64", "f32")}
    own = (ref["status"] & jr.FAILED) == 0
    for k in ("mu", "cov", "z_pred", "S", "innov", "maha", "loglik", "weight_used", "beta0", "innov_comb"):
        per_k = k in ("innov", "maha", "loglik", "weight_used")
        a, b, c = ((x[:, own] if per_k else x[own]) for x in (o["f64"][k], ref[k], o["f32"][k]))
        d = np.abs(a - b) / (1.0 + np.abs(b))
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(d) <= 1e-9, (k, float(np.nanmax(d)))
        assert np.nanmax(np.abs(c - b) / (1.0 + np.abs(b))) <= 2e-2, k


# ------------------------------------------------------------------------------------------------------ the end-to-end scenes
def test_the_end_to_end_scenes_tell_joint_weights_from_per_filter_ones(spe):
    """On the constructed scenes as either engine stores them: every |l| of an allowed pair below the cap, every d^2 5 % clear of the gate, and in
    at least half of the scenes with two or more tracks some pair's joint weight differs from its per-filter weight by 0.05 or
    more -- decided on the reference alone, before any device result exists."""
    mu0, cov0 = spe.synth.pose_initial(CAPACITY)
    c = jr.end_to_end_case(mu0, cov0)
    st = c["starts"]
    assert st[0] == 0 and st[-1] == CAPACITY and np.diff(st).max() == 4 and (np.diff(st) >= 2).sum() >= 300
    for dtype in (np.float64, np.float32):
        s = lambda x: x.astype(dtype).astype(np.float64)   # noqa: E731
        mu, cov, Q, zs = s(c["mu"]), s(c["cov"]), s(c["Q"]), s(c["z_point"])
        pda, beta, beta0, upd, j = jr.reference_chain(on.POSE, mu, cov, zs, Q, st, dtype=dtype)
        pr.conditions(pda, gate=jr.E2E_GATE)
        assert (pda["status"] == 0).all() and (upd["status"] == 0).all() and (j["scene_status"] == 0).all()
        top = jr.largest_log_ratio(s(pda["loglik"]), sr.POSE_POINT, on.POSE, jr.E2E_RULE, dtype, s(pda["maha"]), jr.E2E_GATE)
        share = jr.share_of_scenes_that_differ(pda, beta, st)
        shared = float(((pda["n_gated"] >= 2)).mean())
        print(f"JPDA-INPUTS {np.dtype(dtype).name} spacing={jr.E2E_SPACING} sigma clutter_m3={jr.E2E_RULE.clutter_m3}: max |l|={top:.1f}, "
              f"filters with two or more gated detections {shared:.2f}, share of multi-track scenes with |beta_JPDA - beta_PDA| >= 0.05: {share:.3f}")
        assert top < jr.LOG_RATIO_MAX and share >= 0.5
        assert np.abs(np.nansum(beta, axis=0) + beta0 - 1.0).max() <= (1e-6 if dtype == np.float32 else 1e-12)
        assert not np.array_equal(upd["mu"], mu)
