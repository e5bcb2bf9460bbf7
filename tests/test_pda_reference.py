"""tests/pda_reference.py pinned on the CPU: the NumPy float64 statement of the probabilistic data association update
(include/ukf_batch_pda.h) against what it must reduce to and against itself in the header's whitened form, and the constructed
inputs of tests/test_gpu_pda.py with the conditions they are built to meet.  Tolerance of every check: fp64 on a
12-dimensional state, 1e-12 (1 + |ref|)."""
import numpy as np
import pytest

import associate_reference as ar
import pda_reference as pr
import sensor_meas_cases as smc
import sensor_meas_reference as sr
from engine_support import man_of
from oracle import ukf_numpy as on

TOL = 1e-12
N = 140   # every model id of the cycle, every rotation of the radii and twenty all-outside filters


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and bool((np.abs(a - b)[~np.isnan(b)] <= TOL * (1.0 + np.abs(b[~np.isnan(b)]))).all())


_BATCH = {}


def batch(model, n=N):
    if (model, n) not in _BATCH:
        mu, cov, _ = smc.states(model)
        mu, cov = mu[:n].copy(), cov[:n].copy()
        mount, point, gyro, z, Q = smc.make_inputs(model, mu, np.float64)
        _BATCH[(model, n)] = (man_of(model), mu, cov, mount, point, gyro, z, Q)
    return _BATCH[(model, n)]


def mixed(model, z, ids):
    out = np.zeros((len(ids), 3))
    for mid in sr.ids_of(man_of(model)):
        out[ids == mid] = z[mid][ids == mid]
    return out


def constructed(model, K, ids=None, n=N, **kw):
    man, mu, cov, mount, point, gyro, z, Q = batch(model, n)
    ids = smc.cycling_ids(model, n) if ids is None else ids
    zt = mixed(model, z, np.broadcast_to(ids, (n,)))
    zs, r = pr.constructed_pda(man, mu, cov, ids, zt, Q, mount, point, gyro, K, **kw)
    return ids, zs, r


def run(model, ids, zs, n=N, **kw):
    man, mu, cov, mount, point, gyro, _, Q = batch(model, n)
    kw.setdefault("gate_chi2", pr.GATE)
    return pr.update_pda(man, mu, cov, ids, zs, Q, mount, point, gyro, **kw)


@pytest.mark.parametrize("K", [1, 4, 32])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_constructed_inputs_meet_their_conditions(model, K):
    """every d^2 at least 5 % clear of the gate, the prescribed radii, three of four inside (K = 4), all outside on every 7th
    filter, and the chosen clutter densities put beta_0 inside (0.01, 0.99) on at least half of the filters that have a gated
    candidate"""
    ids, zs, r = constructed(model, K)
    ref = run(model, ids, zs)
    share = pr.conditions(ref)
    live = np.isin(ids, sr.ids_of(man_of(model)))
    print(f"PDA-INPUTS {model} K={K} clutter_m1={pr.CLUTTER_M1} clutter_m3={pr.CLUTTER_M3} share of 0.01 < beta_0 < 0.99: {share:.3f}")
    assert share >= 0.5
    assert np.array_equal(ref["status"] & pr.FAILED, np.where(live, 0, on.ST_INACTIVE))
    assert np.allclose(np.sqrt(ref["maha"][:, live]), r[:, live], rtol=1e-6)
    want = (r * r <= pr.GATE).sum(axis=0)
    assert np.array_equal(ref["n_gated"][live], want[live])
    if K == 4:
        out = np.arange(N) % 7 == 6
        assert (want[~out] == 3).all() and (want[out] == 0).all()
        assert (ref["status"][live & out] == on.ST_REJECTED_GATE).all() and (ref["status"][live & ~out] == 0).all()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_weights_sum_to_one_and_scores_are_the_associations(model):
    ids, zs, _ = constructed(model, 4)
    man, mu, cov, mount, point, gyro, _, Q = batch(model)
    ref = run(model, ids, zs)
    ok = (ref["status"] & pr.FAILED) == 0
    total = ref["beta0"][ok] + ref["beta"][:, ok].sum(axis=0)
    assert (np.abs(total - 1.0) <= TOL).all()
    assert ((ref["beta"][:, ok] == 0.0) == (ref["maha"][:, ok] > pr.GATE)).all()
    asc = ar.associate_sensor(man, mu, cov, ids, zs, Q, mount, point, gyro, gate_chi2=pr.GATE, commit=False)
    for k in ("z_pred", "S"):
        assert close(ref[k], asc[k][0]), k
    for k in ("maha", "loglik"):
        assert close(ref[k], asc[k]), k
    assert close(ref["innov"][:, ok], asc["innov"][:, ok])
    assert np.array_equal(ref["best"], asc["best"]) and np.array_equal(ref["n_gated"], asc["n_gated"])
    # best is the largest weight
    some = ok & (ref["n_gated"] > 0)
    assert np.array_equal(np.argmax(ref["beta"][:, some], axis=0), ref["best"][some])


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_one_candidate_without_clutter_is_the_sensor_update(model):
    """lambda = 1e-300 and K = 1, the gate off: sensor_meas_reference.update_sensor"""
    man, mu, cov, mount, point, gyro, z, Q = batch(model)
    ids = smc.cycling_ids(model, N)
    zt = mixed(model, z, ids)
    rule = pr.RULE._replace(clutter_m1=1e-300, clutter_m3=1e-300)
    got = run(model, ids, zt[None], rule=rule, gate_chi2=-1.0)
    one = sr.update_sensor(man, mu, cov, ids, zt, Q, mount, point, gyro)
    assert np.array_equal(got["status"], one["status"])
    for k in ("mu", "cov", "z_pred", "S"):
        assert close(got[k], one[k]), k
    for k in ("maha", "loglik"):
        assert close(got[k][0], one[k]), k
    live = one["status"] == 0
    assert close(got["innov"][0][live], one["innov"][live]) and close(got["innov_comb"][live], one["innov"][live])
    assert (got["beta"][0][live] == 1.0).all() and (got["beta0"][live] < 1e-30).all()
    assert not np.array_equal(got["mu"][live], mu[live])


def test_equal_candidates_give_the_closed_form():
    """K equal candidates: M = (1 - beta_0) (I - beta_0 y y^T)"""
    rng = np.random.default_rng(3)
    B, D, m, K = 7, 12, 3, 5
    A = rng.standard_normal((B, m, m))
    S = A @ np.swapaxes(A, 1, 2) + 0.1 * np.eye(m)
    G = rng.standard_normal((B, D, D))
    cov = G @ np.swapaxes(G, 1, 2) + np.eye(D)
    C = 0.1 * rng.standard_normal((B, D, m))
    nu1 = rng.standard_normal((B, m))
    nu = np.broadcast_to(nu1, (K, B, m)).copy()
    beta0 = rng.uniform(0.05, 0.95, B)
    beta = np.broadcast_to((1.0 - beta0) / K, (K, B)).copy()
    _, _, M = pr.combine_whitened(cov, C, S, nu, beta, beta0)
    y = np.einsum("bij,bj->bi", np.linalg.inv(np.linalg.cholesky(S)), nu1)
    want = (1.0 - beta0)[:, None, None] * (np.eye(m) - beta0[:, None, None] * y[:, :, None] * y[:, None, :])
    assert close(M, want)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_textbook_and_whitened_forms_agree(model):
    """step 6 written with K = C S^-1 and nu, and with Y = C Ls^-T and y = Ls^-1 nu, on the constructed batch's own numbers"""
    man, mu, cov, mount, point, gyro, z, Q = batch(model)
    mid = sr.POSE_POINT if model == "pose" else sr.ORIENT_NAV_VECTOR
    ids, zs, _ = constructed(model, 4, ids=mid, all_outside=False)
    ref = run(model, mid, zs, commit=False)
    X, _ = on.sigma_points(man, mu, cov)
    Z = sr.h(mid, X, mount[:, None, :], point[:, None, :], gyro[:, None, :])
    C = on.cross_cov_sigma_points(man, on.VECT(3), mu, ref["z_pred"], X, Z)
    S, nu, beta = ref["S"], np.where((ref["beta"] > 0)[:, :, None], ref["innov"], 0.0), ref["beta"]
    a, da, nub = pr.combine_textbook(cov, C @ np.linalg.inv(S), S, nu, beta, ref["beta0"])
    b, db, M = pr.combine_whitened(cov, C, S, nu, beta, ref["beta0"])
    assert close(a, b) and close(da, db) and close(nub, ref["innov_comb"])
    assert (ref["beta0"] > 0.0).all() and not close(b, cov - C @ np.linalg.inv(S) @ np.swapaxes(C, 1, 2))   # the weights matter
    m2, C2, ok = on.apply_delta(man, mu, b, db)
    wet = run(model, mid, zs)
    assert ok.all() and close(wet["mu"], m2) and close(wet["cov"], C2)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_permuted_candidates_permute_the_scores_and_keep_the_state(model):
    ids, zs, _ = constructed(model, 4)
    perm = np.array([2, 0, 3, 1])
    a, b = run(model, ids, zs), run(model, ids, zs[perm])
    for k in ("innov", "maha", "loglik"):
        assert np.array_equal(a[k][perm], b[k], equal_nan=True), k
    assert close(a["beta"][perm], b["beta"])   # (the weights hold the normaliser, a sum in the candidates' order)
    for k in ("mu", "cov", "beta0", "innov_comb", "z_pred", "S"):
        assert close(a[k], b[k]), k
    some = a["best"] >= 0
    assert np.array_equal(perm[b["best"][some]], a["best"][some]) and np.array_equal(a["n_gated"], b["n_gated"])
    assert np.array_equal(a["status"], b["status"])


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_every_candidate_outside_the_gate_keeps_the_state(model):
    man, mu, cov, *_ = batch(model)
    ids, zs, _ = constructed(model, 4)
    ref = run(model, ids, zs, gate_chi2=0.5)   # below every d^2 (the smallest radius is 1)
    live = np.isin(ids, sr.ids_of(man))
    assert (ref["status"][live] == on.ST_REJECTED_GATE).all() and np.array_equal(ref["mu"], mu) and np.array_equal(ref["cov"], cov)
    assert (ref["beta0"][live] == 1.0).all() and (ref["beta"][:, live] == 0.0).all() and (ref["innov_comb"][live] == 0.0).all()
    assert np.isfinite(ref["maha"][:, live]).all() and (ref["best"] == -1).all() and (ref["n_gated"] == 0).all()


def test_status_rules():
    model = "pose"
    n = 12
    man, mu, cov, mount, point, gyro, z, Q = batch(model, n)
    mid = sr.POSE_RANGE
    ids = np.full(n, mid, dtype=np.int32)
    ids[1], ids[2] = -1, sr.ORIENT_VELOCITY
    _, zs, _ = constructed(model, 4, ids=ids, n=n, all_outside=False)
    init = np.ones(n, bool)
    init[0] = False
    zs = zs.copy()
    zs[:, 3, 0] = np.nan            # every candidate absent
    zs[1, 4, 0] = np.nan            # one absent among present ones
    zs[:, 5, 1:] = np.nan           # entries the model does not read
    Qb = Q.copy()
    Qb[6, 0, 0] = np.nan
    covb = cov.copy()
    covb[7] = -np.eye(man.D)
    Qb[8, 0, 0] = -1e6              # S fails
    ref = pr.update_pda(man, mu, covb, ids, zs, Qb, mount, point, gyro, gate_chi2=pr.GATE, initialised=init)
    want = np.zeros(n, dtype=np.uint32)
    want[0], want[1], want[2], want[3], want[6], want[7], want[8] = (on.ST_UNINITIALISED, on.ST_INACTIVE, on.ST_INACTIVE, on.ST_ERR_NONFINITE_MEAS,
                                                                     on.ST_ERR_NONFINITE_MEAS, on.ST_ERR_CHOLESKY, on.ST_ERR_CHOLESKY)
    assert np.array_equal(ref["status"], want)
    bad = want != 0
    assert np.array_equal(ref["mu"][bad], mu[bad]) and np.array_equal(ref["cov"][bad], covb[bad])
    for k in ("z_pred", "S", "beta0"):
        assert np.isnan(ref[k][bad]).all(), k
    for k in ("maha", "loglik", "beta"):
        assert np.isnan(ref[k][:, bad]).all(), k
    assert np.isnan(ref["innov"][:, bad, 0]).all() and np.isnan(ref["innov_comb"][bad, 0]).all()
    m1 = bad & (ids == mid)         # the padding of a refused filter with a model is 0; without a model there is no padding
    assert (ref["innov"][:, m1, 1:] == 0).all() and (ref["innov_comb"][m1, 1:] == 0).all() and np.isnan(ref["innov_comb"][1]).all()
    assert (ref["best"][bad] == -1).all() and (ref["n_gated"][bad] == 0).all()
    # the filter with one absent candidate: NaN there, and the rest act as K - 1 would
    assert np.isnan(ref["beta"][1, 4]) and np.isnan(ref["maha"][1, 4]) and np.isfinite(ref["maha"][[0, 2, 3], 4]).all()
    three = pr.update_pda(man, mu, covb, ids, zs[[0, 2, 3]], Qb, mount, point, gyro, gate_chi2=pr.GATE, initialised=init)
    assert close(ref["mu"][4], three["mu"][4]) and close(ref["cov"][4], three["cov"][4]) and close(ref["beta"][[0, 2, 3], 4], three["beta"][:, 4])
    assert ref["n_gated"][4] == three["n_gated"][4]
    assert ref["status"][5] == 0 and np.isfinite(ref["beta"][:, 5]).all()
    # a float32 combination stays near the float64 one
    f32 = pr.update_pda(man, mu, covb, ids, zs, Qb, mount, point, gyro, gate_chi2=pr.GATE, initialised=init, dtype=np.float32)
    good = want == 0
    assert np.array_equal(f32["status"], want) and np.abs(f32["beta0"][good] - ref["beta0"][good]).max() < 1e-4


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_the_stage_typed_evaluation_in_float64_is_the_reference(model):
    """tests/pda_f32.py with every stage float64 against update_pda (its own mean iteration: 1e-9), and in float32 nearby"""
    import pda_f32
    man, mu, cov, mount, point, gyro, _, Q = batch(model)
    ids, zs, _ = constructed(model, 4)
    ref = run(model, ids, zs)
    inside = np.nan_to_num(ref["beta"], nan=0.0) > 0.0
    keep = (ref["n_gated"] == 0) | (ref["status"] != 0)
    o = {p: pda_f32.pda(model, mu, cov, ids, zs, Q, mount, point, gyro, pr.RULE, inside, keep=keep, prec=p) for p in ("f64", "f32")}
    own = (ref["status"] & pr.FAILED) == 0
    for k in ("mu", "cov", "z_pred", "S", "innov", "maha", "loglik", "beta", "beta0", "innov_comb"):
        a, b = (x[:, own] if k in ("innov", "maha", "loglik", "beta") else x[own] for x in (o["f64"][k], ref[k]))
        d = np.abs(a - b) / (1.0 + np.abs(b))
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(d) <= 1e-9, (k, float(np.nanmax(d)))
        c = (o["f32"][k][:, own] if k in ("innov", "maha", "loglik", "beta") else o["f32"][k][own])
        assert np.nanmax(np.abs(c - b) / (1.0 + np.abs(b))) <= 2e-2, k
