"""The joint association marginals of a scene on the device (ukfb_jpda_scenes_dev / ukfb_jpda_scenes,
include/ukf_batch_jpda.h) against tests/jpda_reference.py on the same inputs AS STORED.  Capacity 1022: ragged scenes of 0 ... 6
tracks straddle the workgroups of four scenes, the last scene ends at the capacity.

Bounds, derived and not measured.  Every sum of the recurrences has positive terms only.  The longest chain is about 600
roundings (32 steps of at most 8 in each of F and G, then the reduction over the wavefront and the division): <= 7e-14
relative.  So on fp64 engines |beta - ref| <= 1e-12 (beta <= 1: a 15-fold margin), likewise beta_0 and free = 1 - sum_i beta_ik
(at most six such terms and the subtraction), and |ln Z - ref| <= 1e-12 (1 + |ref|).  On fp32 engines the solve is the same fp64
solve and the store rounds once: |beta - fl32(ref)| <= 2^-23, one fp32 rounding of a value <= 1 plus the above; free and ln Z
are stored as doubles and keep the fp64 bound.  Status words, the NaN pattern and the exact zeros are equal to the reference's.
tests/test_jpda_reference.py asserts that every |l| of the random inputs here is below the cap of 100."""
import numpy as np
import pytest
import torch

import jpda_reference as jr
import pda_reference as pr
from engine_support import man_of, new_engine, same_snapshot, snapshot, tdt
from probe_support import LDS_PATTERNS, lds_poison

pytestmark = pytest.mark.gpu

N = 1022
GUARD = 96
PRECS = [("f64", 0), ("f32", 1)]
TOL64 = 1e-12
TOL32 = 2.0 ** -23
F_SENTINEL, U32_SENTINEL = -7.0, 0x7FFF
OUTPUTS = ("beta", "beta0", "free", "log_z", "scene_status")

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


def run(spe, e, loglik, maha, starts=None, models=0, gate=-1.0, tracks_per_scene=0, scenes=None, want=OUTPUTS, rule=pr.RULE):
    """loglik, maha [K, N] as the engine stores them (maha may be None); starts: offsets or None (uniform mode); models: an id or
    an array [N].  Returns the outputs as NumPy arrays (float64), and "guards": True while every guard region holds its sentinel."""
    K = loglik.shape[0]
    if scenes is None:
        scenes = len(starts) - 1 if starts is not None else -(-N // tracks_per_scene)
    t = tdt(e)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x.astype(e.dtype))).cuda()   # noqa: E731
    ll_t, d2_t = up(loglik), None if maha is None else up(maha)
    starts_t = None if starts is None else torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int32)).cuda()
    ids_t = None if np.isscalar(models) else torch.from_numpy(np.ascontiguousarray(models, dtype=np.int32)).cuda()
    spec = {"beta": (K * N, t, F_SENTINEL), "beta0": (N, t, F_SENTINEL), "free": (scenes * K, torch.float64, F_SENTINEL),
            "log_z": (scenes, torch.float64, F_SENTINEL), "scene_status": (scenes, torch.int32, U32_SENTINEL)}
    bufs = {k: guarded(*spec[k]) for k in want}
    torch.cuda.synchronize()
    e.jpda_scenes_dev(K, ll_t, spe.PdaRule(*rule), scenes, scene_start_dev=starts_t, tracks_per_scene=tracks_per_scene, maha_dev=d2_t,
                      gate=gate, model=int(models) if ids_t is None else 0, model_dev=ids_t, **{k: v[1] for k, v in bufs.items()})
    e.sync()
    out = {k: v[1].cpu().numpy().astype(np.float64 if k != "scene_status" else np.uint32) for k, v in bufs.items()}
    if "beta" in out:
        out["beta"] = out["beta"].reshape(K, N)
    if "free" in out:
        out["free"] = out["free"].reshape(scenes, K)
    out["guards"] = all(bool((w[:GUARD] == spec[k][2]).all()) and bool((w[GUARD + spec[k][0]:] == spec[k][2]).all()) for k, (w, _) in bufs.items())
    return out


def check(name, e, model, out, loglik, maha, starts, models, gate, rule=pr.RULE):
    """a launch against the reference on the same inputs; returns the reference"""
    ref = jr.jpda_scenes(man_of(model), loglik, maha, starts, models, rule, gate, e.dtype, sentinel=F_SENTINEL)
    assert np.array_equal(out["scene_status"], ref["scene_status"])
    f32 = e.dtype == np.float32
    tol = TOL32 if f32 else TOL64
    worst = {}
    for k in ("beta", "beta0"):
        want = ref[k].astype(np.float32).astype(np.float64) if f32 else ref[k]
        assert np.array_equal(np.isnan(out[k]), np.isnan(want)), (name, k)                       # NaN where loglik is not finite
        assert np.array_equal(out[k] == F_SENTINEL, want == F_SENTINEL), (name, k)               # nothing outside the good scenes
        assert np.array_equal(out[k] == 0.0, want == 0.0), (name, k)                             # exact zeros where the pair is forbidden
        fin = ~np.isnan(want)
        worst[k] = float(np.abs(out[k][fin] - want[fin]).max())
    solved = ref["scene_status"] == jr.OK
    assert (out["free"][~solved] == F_SENTINEL).all() and (out["log_z"][~solved] == F_SENTINEL).all()
    worst["free"] = float(np.abs(out["free"][solved] - ref["free"][solved]).max())
    worst["log_z"] = float((np.abs(out["log_z"][solved] - ref["log_z"][solved]) / (1.0 + np.abs(ref["log_z"][solved]))).max())
    print(f"PARITY jpda/{name} " + " ".join(f"max_d{k}={v:.3e}" for k, v in worst.items()) + f" tol={tol:.3e} tol64={TOL64:.1e}")
    assert worst["beta"] <= tol and worst["beta0"] <= tol and worst["free"] <= TOL64 and worst["log_z"] <= TOL64, (name, worst)
    return ref


# ---------------------------------------------------------------------------------------------------------- 1: ragged scenes
@pytest.mark.parametrize("name,prec", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("K,seed", [(1, 11), (5, 12), (32, 13)])
def test_ragged_scenes(spe, name, prec, K, seed):
    """scene sizes cycling through 0 ... 6 from slot 5 to the capacity; 20 % of the pairs NaN or +-Inf in loglik, 5 % NaN in maha
    alone; the gate off and on; model ids with m = 1 and m = 3, -1 and an id of the other engine cycling through the tracks"""
    e = engine(spe, "pose", prec)
    starts = jr.ragged_starts(N)
    ids = jr.mixed_models(man_of("pose"), N)
    ll, d2 = jr.synthetic_scores(seed, N, K, e.dtype)
    for gate, maha in ((-1.0, None), (-1.0, d2), (jr.SYNTH_GATE, d2)):
        out = run(spe, e, ll, maha, starts, ids, gate)
        assert out["guards"]
        ref = check(f"{name}/K={K}/gate={gate:g}", e, "pose", out, ll, maha, starts, ids, gate)
        assert (out["beta"][:, :5] == F_SENTINEL).all() and (out["beta0"][:5] == F_SENTINEL).all() and (out["beta0"][5:] != F_SENTINEL).all()
        total = np.nansum(out["beta"][:, 5:], axis=0) + out["beta0"][5:]
        assert np.abs(total - 1.0).max() <= (K + 1) * (TOL32 if prec else TOL64)
        assert (out["free"] >= -TOL64).all() and (out["free"] <= 1.0).all() and (ref["log_z"] >= 0.0).all()
        assert (out["beta"] > 0.0).sum() > 0 and (gate < 0 or (out["beta"] == 0.0).sum() > 0)


def test_orientation_engine_plumbing(spe):
    e = engine(spe, "orient", 1)
    starts = jr.ragged_starts(N)
    ids = jr.mixed_models(man_of("orient"), N)
    ll, d2 = jr.synthetic_scores(21, N, 5, e.dtype)
    out = run(spe, e, ll, d2, starts, ids, jr.SYNTH_GATE)
    assert out["guards"]
    check("orient/f32/K=5", e, "orient", out, ll, d2, starts, ids, jr.SYNTH_GATE)


# ------------------------------------------------------------------------------------------------------------- 2: the cap
@pytest.mark.parametrize("name,prec", PRECS, ids=[p[0] for p in PRECS])
def test_six_by_thirty_two_with_every_log_ratio_at_the_cap(spe, name, prec):
    """every l far above 100: psi = e^100 for all 192 pairs of a scene, in every scene slot of a workgroup; the sums stay finite"""
    e = engine(spe, "pose", prec)
    ll = np.full((32, N), 500.0)
    out = run(spe, e, ll, None, None, 0, -1.0, tracks_per_scene=6)
    assert out["guards"] and np.isfinite(out["beta"]).all() and np.isfinite(out["log_z"]).all()
    starts = jr.uniform_starts(N, 6)
    one = jr.jpda_scenes(man_of("pose"), ll[:, :6], None, np.array([0, 6]), 0, dtype=e.dtype)
    full = np.diff(starts) == 6
    assert full.sum() == 170 and (out["scene_status"] == jr.OK).all()
    tol = TOL32 if prec else TOL64
    want = one["beta"].astype(e.dtype).astype(np.float64)
    worst = max(float(np.abs(out["beta"][:, a:a + 6] - want).max()) for a in starts[:-1][full])
    worst_z = float(np.abs(out["log_z"][full] - one["log_z"][0]).max() / (1.0 + one["log_z"][0]))
    print(f"PARITY jpda/{name}/capped 6 x 32 max_dbeta={worst:.3e} tol={tol:.3e} max_dlog_z={worst_z:.3e} ln Z={one['log_z'][0]:.3f}")
    assert worst <= tol and worst_z <= TOL64
    assert all(np.array_equal(out["beta"][:, a:a + 6], out["beta"][:, :6]) for a in starts[:-1][full])   # every position: the same bits
    check(f"{name}/capped", e, "pose", out, ll, None, starts, 0, -1.0)


# --------------------------------------------------------------------------------------------- 3: bad and too-large scenes
@pytest.mark.parametrize("name,prec", PRECS, ids=[p[0] for p in PRECS])
def test_bad_and_too_large_scenes_write_their_status_and_nothing_else(spe, name, prec):
    """Offsets the kernel cannot trust (non-monotone, an end beyond the capacity, a negative start, 33 tracks) and well-formed
    scenes of 7, 8, 9 and 32 tracks between good ones.  No access is made with a bad offset: nothing here faults."""
    e = engine(spe, "pose", prec)
    #                  good     7        8        9        good     BAD (back) TOO (32) BAD (33)  good      BAD (beyond) BAD (neg) good
    starts = np.array([100, 105, 112,    120,     129,     133,     10,        42,      75,       78,       N + 40,      -3,       150, 156], dtype=np.int32)
    ids = jr.mixed_models(man_of("pose"), N)
    ll, d2 = jr.synthetic_scores(41, N, 6, e.dtype)
    out = run(spe, e, ll, d2, starts, ids, jr.SYNTH_GATE)
    assert out["guards"]
    ref = check(f"{name}/bad-scenes", e, "pose", out, ll, d2, starts, ids, jr.SYNTH_GATE)
    assert ref["scene_status"].tolist() == [0, 2, 2, 2, 0, 1, 2, 1, 0, 1, 1, 1, 0]
    written = jr.covered(starts, N)
    assert written.sum() == 5 + 4 + 3 + 6 and (out["beta0"][~written] == F_SENTINEL).all() and (out["beta"][:, ~written] == F_SENTINEL).all()
    assert (out["beta0"][written] != F_SENTINEL).all()
    # the host-array form knows the offsets and refuses the bad ones before any launch; too-large ones it lets through
    with pytest.raises(spe.UkfbError, match="code 4"):
        e.jpda_scenes(ll, spe.PdaRule(*pr.RULE), scene_start=starts, maha=d2, gate=jr.SYNTH_GATE, model=ids)
    ok_starts = np.array([100, 105, 112, 120, 129, 133], dtype=np.int32)
    got = e.jpda_scenes(ll, spe.PdaRule(*pr.RULE), scene_start=ok_starts, maha=d2, gate=jr.SYNTH_GATE, model=ids)
    assert got["scene_status"].tolist() == [0, 2, 2, 2, 0]
    assert np.array_equal(got["beta"][:, 100:105], out["beta"][:, 100:105], equal_nan=True) and np.isnan(got["beta"][:, 105:129]).all()
    assert np.array_equal(got["beta0"][129:133], out["beta0"][129:133]) and np.isnan(got["beta0"][:100]).all() and np.isnan(got["log_z"][1:4]).all()


# -------------------------------------------------------------------------------------------- 4: uniform mode, host-array form
@pytest.mark.parametrize("name,prec", PRECS, ids=[p[0] for p in PRECS])
def test_uniform_mode_equals_offsets_mode_and_the_host_form(spe, name, prec):
    e = engine(spe, "pose", prec)
    ids = jr.mixed_models(man_of("pose"), N)
    rule = spe.PdaRule(*pr.RULE)
    for T0, K in ((1, 3), (2, 4), (4, 8), (6, 32)):
        ll, d2 = jr.synthetic_scores(60 + T0, N, K, e.dtype)
        starts = jr.uniform_starts(N, T0)
        by_offsets = run(spe, e, ll, d2, starts, ids, jr.SYNTH_GATE)
        uniform = run(spe, e, ll, d2, None, ids, jr.SYNTH_GATE, tracks_per_scene=T0)
        assert uniform["guards"] and by_offsets["guards"]
        assert all(np.array_equal(uniform[k], by_offsets[k], equal_nan=True) for k in OUTPUTS)
        check(f"{name}/uniform T0={T0} K={K}", e, "pose", uniform, ll, d2, starts, ids, jr.SYNTH_GATE)
        # fewer scenes than fit: the rest is not written
        few = run(spe, e, ll, d2, None, ids, jr.SYNTH_GATE, tracks_per_scene=T0, scenes=3)
        assert np.array_equal(few["beta"][:, :3 * T0], uniform["beta"][:, :3 * T0], equal_nan=True) and (few["beta"][:, 3 * T0:] == F_SENTINEL).all()
        assert np.array_equal(few["free"], uniform["free"][:3])
        # a single output is enough
        only = run(spe, e, ll, d2, None, ids, jr.SYNTH_GATE, tracks_per_scene=T0, want=("log_z",))
        assert np.array_equal(only["log_z"], uniform["log_z"]) and only["guards"]
    # the host-array form: doubles in, the same answer; slots no scene covers read NaN
    ll, d2 = jr.synthetic_scores(71, N, 5, e.dtype)
    starts = jr.ragged_starts(N)
    dev = run(spe, e, ll, d2, starts, ids, jr.SYNTH_GATE)
    got = e.jpda_scenes(ll, rule, scene_start=starts, maha=d2, gate=jr.SYNTH_GATE, model=ids)
    assert np.array_equal(got["beta"][:, 5:], dev["beta"][:, 5:], equal_nan=True) and np.isnan(got["beta"][:, :5]).all()
    assert np.array_equal(got["beta0"][5:], dev["beta0"][5:]) and all(np.array_equal(got[k], dev[k]) for k in ("free", "log_z", "scene_status"))
    got = e.jpda_scenes(ll, rule, tracks_per_scene=4, model=2)
    ref = run(spe, e, ll, None, None, 2, -1.0, tracks_per_scene=4)
    assert all(np.array_equal(got[k], ref[k], equal_nan=True) for k in OUTPUTS)
    # argument errors, decided before any launch
    for kw, code in ((dict(tracks_per_scene=0), 4), (dict(tracks_per_scene=7), 4), (dict(tracks_per_scene=4, scenes=257), 4),
                     (dict(tracks_per_scene=4, scenes=-1), 4), (dict(tracks_per_scene=4, gate=16.0), 1)):
        with pytest.raises(spe.UkfbError, match=f"code {code}"):
            e.jpda_scenes(ll, rule, **kw)
    with pytest.raises(spe.UkfbError, match="code 1"):
        e.jpda_scenes(ll, spe.PdaRule(*pr.RULE._replace(p_detect=1.0, p_gate_m3=1.0)), tracks_per_scene=4)
    ll_t = torch.from_numpy(ll.astype(e.dtype)).cuda()
    with pytest.raises(spe.UkfbError, match="code 1"):
        e.jpda_scenes_dev(5, ll_t, rule, 3, tracks_per_scene=4)   # every output NULL
    e.jpda_scenes_dev(5, ll_t, rule, 0, tracks_per_scene=4, beta0=ll_t)   # scenes = 0: nothing launched, nothing written
    e.sync()
    assert np.array_equal(ll_t.cpu().numpy().astype(np.float64), ll, equal_nan=True)


# ------------------------------------------------------------------------------------------- 5: read-only, leftovers in LDS
@pytest.mark.parametrize("name,prec", PRECS, ids=[p[0] for p in PRECS])
def test_read_only_and_independent_of_lds_leftovers(spe, name, prec):
    e = engine(spe, "pose", prec)
    starts = jr.ragged_starts(N)
    ids = jr.mixed_models(man_of("pose"), N)
    ll, d2 = jr.synthetic_scores(81, N, 32, e.dtype)
    before = snapshot(e, noise_of=(0, N - 1))
    clean = run(spe, e, ll, d2, starts, ids, jr.SYNTH_GATE)
    assert same_snapshot(before, snapshot(e, noise_of=(0, N - 1)))
    check(f"{name}/read-only", e, "pose", clean, ll, d2, starts, ids, jr.SYNTH_GATE)
    poison = lds_poison()
    for pattern in (LDS_PATTERNS[0], LDS_PATTERNS[2]):   # a float NaN; all ones: a NaN in both precisions
        assert poison(pattern) == 0
        out = run(spe, e, ll, d2, starts, ids, jr.SYNTH_GATE)
        assert all(np.array_equal(out[k], clean[k], equal_nan=True) for k in OUTPUTS), hex(pattern)
    # the same scene at another position of its workgroup: the same bits
    shifted = run(spe, e, np.roll(ll, 1, axis=1), np.roll(d2, 1, axis=1), np.concatenate(([0], starts + 1))[:-1].astype(np.int32),
                  np.roll(ids, 1), jr.SYNTH_GATE)
    assert np.array_equal(shifted["beta"][:, 6:N - 6], clean["beta"][:, 5:N - 7], equal_nan=True)
    assert np.array_equal(shifted["log_z"][1:-2], clean["log_z"][:-3])
