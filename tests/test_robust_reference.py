"""Pins for tests/robust_reference.py, the NumPy statement of the robust sensor-frame update (include/ukf_batch_robust.h) the
GPU tests compare with, and the conditions of the constructed inputs those tests rely on.

Inputs: sensor_meas_cases.states(model) with make_inputs; the innovation of filter i replaced by Ls u rho, rho = (0.5, 1.5, 4,
8, 30, 300)[i mod 6] (robust_reference.contaminate, seed 7).  On these states: at most 8 Newton steps (POSE_POINT,
ORIENT_NAV_VECTOR), agreement with the bisected root within 7.6e-13, elasticity eta >= 0.064, cond(S(root)) <= 6.0e2, lambda
up to 1.2e8."""
import numpy as np
import pytest

import robust_reference as rr
import sensor_meas_reference as sr
from engine_support import man_of
from sensor_meas_cases import N, cycling_ids, make_inputs, states

_CASES = {}


def batch(model):
    """-> per model id: dict(z contaminated, raw = update_sensor at lambda = 1, and for the outliers out: Sz, Q, nu, c2, root)"""
    if model not in _CASES:
        mu, cov, _ = states(model)
        mount, point, gyro, z, Q = make_inputs(model, mu, np.float64)
        man = man_of(model)
        per = {}
        for mid in sr.ids_of(man):
            zc = rr.contaminate(man, mu, cov, mid, z[mid], Q, mount, point, gyro)
            raw = sr.update_sensor(man, mu, cov, mid, zc, Q, mount, point, gyro)
            assert (raw["status"] == 0).all()
            c2 = rr.CHI2_M1 if sr.meas_dim(mid) == 1 else rr.CHI2_M3
            out = raw["maha"] > c2
            Sz, Qe, nu = rr.embed(np.full(int(out.sum()), mid), raw["S"][out], Q[out], raw["innov"][out])
            per[mid] = dict(z=zc, raw=raw, out=out, Sz=Sz, Q=Qe, nu=nu, c2=c2, root=rr.solve_scale(Sz, Qe, nu, c2, rr.MATCH))
        _CASES[model] = (man, mu, cov, mount, point, gyro, Q, per)
    return _CASES[model]


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_the_constructed_radius_is_the_raw_distance(model):
    *_, per = batch(model)
    rho = np.array(rr.RHO)[np.arange(N) % 6]
    for mid, b in per.items():
        assert np.allclose(b["raw"]["maha"], rho ** 2, rtol=1e-9), mid
        assert np.array_equal(b["out"], rho >= 4.0)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_thresholds_out_of_reach_give_update_sensor_array_for_array(model):
    man, mu, cov, mount, point, gyro, Q, per = batch(model)
    ids = cycling_ids(model, N)
    z = np.zeros((N, 3))
    for mid, b in per.items():
        z[ids == mid] = b["z"][ids == mid]
    for gate in (-1.0, rr.GATE):
        ref = sr.update_sensor(man, mu, cov, ids, z, Q, mount, point, gyro, gate_chi2=gate)
        got = rr.update_robust(man, mu, cov, ids, z, Q, mount, point, gyro, rule=rr.rule(chi2_m1=1e30, chi2_m3=1e30), gate_chi2=gate)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (gate, k)
        scored = ~np.isnan(ref["maha"])
        assert (got["scale"][scored] == 1.0).all() and np.isnan(got["scale"][~scored]).all() and (got["iterations"] == 0).all()
        assert np.array_equal(got["maha0"], ref["maha"], equal_nan=True)
    assert ((ref["status"] & 0x200) != 0).sum() >= N // 5   # rho = 30, 300: a third of the rows that have a model (5 of 7, 3 of 5)


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_newton_against_the_independent_root(model):
    *_, per = batch(model)
    worst = 0
    for mid, b in per.items():
        it, steps = rr.newton_iterates(b["Sz"], b["Q"], b["nu"], b["c2"], tol=1e-13, max_iter=16)
        root = b["root"]
        rel = np.abs(it[:, -1] - root) / root
        print(f"NEWTON {sr.NAMES[mid]} rows={root.size} steps max={steps.max()} mean={steps.mean():.2f} max|lam - root|/root={rel.max():.2e} "
              f"lam max={root.max():.3e}")
        assert rel.max() <= 1e-9, mid
        assert (it <= root[:, None] * (1 + 1e-12)).all(), mid          # the iterates never pass the root ...
        assert (np.diff(it, axis=1) >= 0).all() and (it[:, 0] == 1.0).all()   # ... and rise monotonically from 1
        assert steps.max() <= 8, (mid, steps.max())                    # half of the cap the GPU tests use
        if sr.meas_dim(mid) == 1:
            assert (steps == 1).all()                                  # m = 1: one step is exact
        f, _ = rr.evaluate(b["Sz"], b["Q"], b["nu"], it[:, -1])
        assert (np.abs(f - b["c2"]) <= 1e-9 * b["c2"]).all()
        worst = max(worst, int(steps.max()))
    assert worst >= 3   # the loop is exercised


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_separation_and_conditioning(model):
    *_, per = batch(model)
    eta_min, cond_max = np.inf, 0.0
    for mid, b in per.items():
        if mid in rr.CLAMP_MODELS[model]:   # the batches the GPU test clamps: one model's each
            scale_max = rr.pick_scale_max(b["root"])
            assert (b["root"] > 1.1 * scale_max).any() and (b["root"] < 0.9 * scale_max).any(), mid
        d0 = b["raw"]["maha"]
        assert not (np.abs(d0 - b["c2"]) <= 0.1 * b["c2"]).any() and not (np.abs(d0 - rr.GATE) <= 0.1 * rr.GATE).any()
        f, g = rr.evaluate(b["Sz"], b["Q"], b["nu"], b["root"])
        eta = b["root"] * g / f
        m = sr.meas_dim(mid)
        S = (b["Sz"] + b["root"][:, None, None] * b["Q"])[:, :m, :m]
        eta_min, cond_max = min(eta_min, eta.min()), max(cond_max, np.linalg.cond(S).max())
    print(f"CONDITIONS {model} eta min={eta_min:.3e} cond(S) max={cond_max:.3e}")
    assert eta_min >= 0.05 and cond_max <= 2000.0
    # what makes a direct comparison of lambda at 1e-9 legitimate in fp64
    assert (1e-13 + 64 * 2.0 ** -52 * cond_max) / eta_min < 6e-10


def test_huber_is_the_closed_form_and_bounds_the_update():
    man, mu, cov, mount, point, gyro, Q, per = batch("pose")
    mid = sr.POSE_POINT
    b = per[mid]
    r = rr.rule(mode=rr.HUBER)
    got = rr.update_robust(man, mu, cov, mid, b["z"], Q, mount, point, gyro, rule=r)
    d0 = b["raw"]["maha"]
    want = np.where(b["out"], np.sqrt(d0 / b["c2"]), 1.0)
    assert np.array_equal(got["scale"], want) and (got["iterations"] == 0).all() and (got["status"] == 0).all()
    assert np.allclose(rr.solve_scale(b["Sz"], b["Q"], b["nu"], b["c2"], rr.HUBER), want[b["out"]], rtol=1e-12, atol=0)
    # the distance of an outlier falls, but not to c^2; MATCH brings it there
    assert (got["maha"][b["out"]] < d0[b["out"]]).all()
    match = rr.update_robust(man, mu, cov, mid, b["z"], Q, mount, point, gyro, rule=rr.rule())
    assert np.allclose(match["maha"][b["out"]], b["c2"], rtol=1e-9)
    assert np.array_equal(match["maha"][~b["out"]], d0[~b["out"]]) and (match["iterations"][~b["out"]] == 0).all()


def test_gate_clamp_and_cap_in_the_reference():
    man, mu, cov, mount, point, gyro, Q, per = batch("pose")
    mid = sr.POSE_VELOCITY
    b = per[mid]
    scale_max = rr.pick_scale_max(b["root"])
    got = rr.update_robust(man, mu, cov, mid, b["z"], Q, mount, point, gyro, rule=rr.rule(scale_max=scale_max), gate_chi2=rr.GATE)
    rho = np.array(rr.RHO)[np.arange(N) % 6]
    gated = rho >= 30
    assert np.array_equal(got["status"], np.where(gated, 0x200, 0))
    assert np.array_equal(got["mu"][gated], mu[gated]) and (got["scale"][gated] == 1.0).all() and (got["iterations"][gated] == 0).all()
    free = rr.update_robust(man, mu, cov, mid, b["z"], Q, mount, point, gyro, rule=rr.rule(scale_max=scale_max))
    clamped = free["scale"] == scale_max
    assert clamped.any() and (free["maha"][clamped] > b["c2"]).all() and (free["status"] == 0).all()
    assert not np.array_equal(free["mu"][clamped], mu[clamped])
    one = rr.update_robust(man, mu, cov, mid, b["z"], Q, mount, point, gyro, rule=rr.rule(max_iter=1))
    it, _ = rr.newton_iterates(b["Sz"], b["Q"], b["nu"], b["c2"], max_iter=1)
    assert it.shape[1] == 2 and np.array_equal(one["scale"][b["out"]], it[:, 1]) and (one["iterations"][b["out"]] == 1).all()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_plain_fp32_bounds_come_from_the_float32_evaluation(model):
    """the bounds a plain fp32 engine's lambda and residual are held to (tests/test_gpu_robust.py forms them on its own batch
    in the same way): M_FEAT times what the all-float32 evaluation leaves, floor 20 * 2^-24.  The lines are
    profiles/robust_parity.txt.  Sanity, from eps_32 cond(S) / eta = 6e-8 * 2000 / 0.06 = 2e-3: every distance is below it."""
    import feature_scaled_parity as fsp
    man, mu, cov, mount, point, gyro, Q, per = batch(model)
    f = lambda a: None if a is None else a.astype(np.float32).astype(np.float64)   # noqa: E731
    for mid, b in per.items():
        for mname, mode in (("match", rr.MATCH), ("huber", rr.HUBER)):
            d = rr.f32_distances(model, f(mu), f(cov), mid, f(b["z"]), f(Q), f(mount), f(point), f(gyro), rr.rule(mode=mode, tol=2e-6))
            lam_bound = max(fsp.M_FEAT * d["d_lam"], rr.FLOOR_F32)
            line = f"BOUND {model}/f32/{mname}/{sr.NAMES[mid]} rows={int(d['rows'].sum())} d_32(lambda)={d['d_lam']:.3e} bound={lam_bound:.3e}"
            if mode == rr.MATCH:
                line += f" d_32(residual)={d['d_resid']:.3e} bound={max(fsp.M_FEAT * d['d_resid'], rr.FLOOR_F32):.3e}"
                assert 0.0 <= d["d_resid"] < 2e-3
            print(line)
            assert 0.0 < d["d_lam"] < 2e-3 and d["rows"].sum() == 680
