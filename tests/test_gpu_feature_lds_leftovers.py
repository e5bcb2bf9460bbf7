"""No feature kernel may depend on LDS it did not write itself: tests/test_gpu_lds_leftovers.py for the row-layout kernels.

Every feature kernel keeps each filter in a slice of the workgroup's dynamic LDS described by a map of ukf_host.hpp (RowSlice);
the maps are full of scalars no lane writes: a mean region of 16 holds S = 13 or 14, factor columns of stride ROW_LS = 14 hold
D = 12 or 13, 16 reciprocal pivots serve D, the packed covariance is padded to even, a rotation takes 9 (+ 1), a slice is rounded
up to four.  "Every scalar a kernel reads is one it wrote: the pads are never read" (ukf_host.hpp) is held here: the LDS of
every compute unit is filled with a NaN, an Inf, an all-ones and a zero pattern (tests/cpp/lds_poison.hip) right in front of the
one call, and every output of the call and the engine's whole snapshot must have the bits of the run that found whatever the
test before left there.  No reference and no tolerance: the parity of each feature is its own file's business.

Every case: 253 filters (63 workgroups of four and one of a single filter with three repeat rows), brought to a real state by
two cycles; filter DEAD is never initialised, filter BAD stores a NaN in one covariance entry (its factorisation fails) -- the two
share wavefront 5 with healthy rows -- and where the call has them every seventh filter is masked out, filter NANZ gets a
non-finite sample and filter GATED one beyond gate_chi2.  Every input is uploaded and every output allocated, and prefilled with
NaN (integers: -1), before the poison; the engine is rebuilt bit for bit for every pattern.

The instrument sees what it should (profiles/lds_leftovers.txt): the poison survives into the next kernel's allocation whole, and
the sensor-frame kernel built once with T(0) * PKF[PK] added to its published mean (the pad behind OrientationState's packed
covariance) fails test_sensor_frame[orient-f64] at the all-ones pattern, the only one of the three that is a NaN as a double."""
import numpy as np
import pytest
import torch

import bank_reference as br
import bearing_reference as bear
import relative_cases as rc
import robust_reference as rob
import sensor_meas_cases as smc
import sensor_meas_reference as sr
import state_meas_reference as smr
from engine_support import ACC_COV, Case, cycled_engine, man_of, new_engine, pack, same, same_snapshot, snapshot, stored
from oracle import ukf_numpy as on
from probe_support import LDS_PATTERNS, lds_poison

pytestmark = pytest.mark.gpu

N = 253
MODES = {"f64": (0, 0), "f32": (1, 0), "f32w": (1, 1)}   # (precision, wide_arithmetic): f32w = the fp64 instantiation on fp32 storage
CELLS = [(model, mode) for model in ("pose", "orient") for mode in MODES]
BAD, DEAD, NANZ, GATED = 21, 22, 30, 35     # 20 ... 23 are one wavefront: 20 and 23 stay healthy
GATE = 1e4
BEARING_GATE = 100.0   # the orientation sigma of 0.05 rad bounds the d^2 of a direction: pi^2 / 0.05^2 = 4e3
STEPS, SLOTS, FIRST = 6, 8, 5               # the history window wraps: slots 5, 6, 7, 0, 1, 2
ST_NONFINITE, ST_CHOLESKY, ST_UNINIT, ST_INACTIVE, ST_REJECTED, ST_WEIGHTS = 1 << 4, 1 << 5, 1 << 7, 1 << 8, 1 << 9, 1 << 10
cells = pytest.mark.parametrize("model,mode", CELLS, ids=[f"{a}-{b}" for a, b in CELLS])


# ---------------------------------------------------------------------------------------------------------------- the case
_BASE = {}


def base(spe, model, mode, n=N, state=None):
    """the downloaded state of an engine after two real cycles (or `state`, stored once), and the inputs it latches"""
    key = (model, mode, n, state is None)
    if key not in _BASE or state is not None:
        prec, wide = MODES[mode]
        c = Case()
        c.model, c.mode, c.n, c.prec, c.wide = model, mode, n, prec, wide
        if state is None:
            e = cycled_engine(spe, model, n, prec, wide)
        else:
            e = new_engine(spe, model, n, prec, wide)
            e.initialize(*state)
        c.mu, c.cov, _ = e.state()
        c.dtype, c.S, c.D, c.PK = e.dtype, e.S, e.D, e.PK
        e.close()
        c.T = torch.float64 if prec == 0 else torch.float32
        sy = spe.synth
        if model == "pose":
            c.in_a, c.in_b = sy.pose_cycle_inputs(n, 2, c.mu[:, :3])[0], np.zeros((n, 3))
        else:
            c.in_b, c.in_a = sy.orient_cycle_inputs(n, 2, c.mu[:, 0:4])[:2]   # (gyro, acc)
        c.last = np.arange(1, n + 1, dtype=np.int64) * 1000 + 7
        c.bad, c.dead = BAD, DEAD
        if state is not None:
            return c
        _BASE[key] = c
    return _BASE[key]


def planted(spe, c, **cfg):
    """a fresh engine with the case's state bit for bit, filter c.dead left uninitialised and a NaN in filter c.bad's covariance"""
    e = new_engine(spe, c.model, c.n, c.prec, c.wide, **cfg)
    cov = c.cov.copy()
    cov[c.bad, 2, 1] = cov[c.bad, 1, 2] = np.nan
    for lo, hi in ((0, c.dead), (c.dead + 1, c.n)):
        e.initialize(c.mu[lo:hi], cov[lo:hi], first=lo)
    if c.model == "pose":
        e.set_acceleration(c.in_a, ACC_COV)
    else:
        e.set_orient_inputs(c.in_b, c.in_a)
    e.set_last_measurement_time(c.last)
    return e


def up(c, x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype or c.T)


def nans(c, *shape):
    return torch.full(shape, float("nan"), dtype=c.T, device="cuda")


def ints(*shape, dtype=torch.int32):
    return torch.full(shape, -1, dtype=dtype, device="cuda")


def every_seventh(n):
    return np.arange(n) % 7 == 3


# ------------------------------------------------------------------------------------------------------------ the instrument
def leftovers(spe, c, call, outs, name, prepare=None, **cfg):
    """call(e) once after every pattern on an engine rebuilt for it (prepare(e): the last part of the rebuilding) -> (outputs,
    snapshot before, snapshot after) of the un-poisoned run, every other run's outputs and snapshot asserted equal to it bit for
    bit (NaN equal to NaN)"""
    poison = lds_poison()
    first = {k: v.clone() for k, v in outs.items()}   # the sentinels; for an in-place call its input
    runs = []
    for pat in (None,) + LDS_PATTERNS:
        e = planted(spe, c, **cfg)
        if prepare is not None:
            prepare(e)
        for k, v in outs.items():
            v.copy_(first[k])
        before = snapshot(e, (0, c.n - 1))
        e.sync()
        torch.cuda.synchronize()
        if pat is not None:
            assert poison(pat) == 0
        call(e)
        e.sync()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        runs.append((got, before, snapshot(e, (0, c.n - 1))))
        e.close()
    got0, before0, after0 = runs[0]
    for pat, (got, before, after) in zip(LDS_PATTERNS, runs[1:]):
        assert same_snapshot(before, before0), (name, "the rebuilt engine")
        differ = [k for k in outs if not same(got, got0, (k,))]
        assert not differ, (name, hex(pat), differ, [int(np.nonzero(~_eq(got[k], got0[k]))[0][0]) for k in differ])
        assert same_snapshot(after, after0), (name, hex(pat), "snapshot")
    return got0, before0, after0


def _eq(a, b):
    return (a == b) | ((a != a) & (b != b))


def judge(c, name, got, before, after, commit, inactive=None, nonfinite=(), gated=(), per_filter=(), per_candidate=(), st=None, dead=None,
          bad=None, failing=ST_CHOLESKY | ST_NONFINITE):
    """the run was not trivial: the planted rows carry their bits, most other rows are 0 and their outputs finite, the committed
    state moved (commit) or the whole snapshot kept its bits (read-only; commit None: the caller looks)"""
    st = (got["status"] if st is None else st).astype(np.uint32)
    n = st.size
    dead = [c.dead] if dead is None else dead
    bad = [c.bad] if bad is None else bad
    inactive = np.zeros(n, bool) if inactive is None else np.asarray(inactive, bool)
    assert all(st[i] & ST_UNINIT for i in dead), (name, st[dead])
    assert all(st[i] & failing for i in bad), (name, st[bad])
    assert ((st[inactive] & ST_INACTIVE) != 0).all(), (name, np.unique(st[inactive]))
    assert all(st[i] & ST_NONFINITE for i in nonfinite), (name, [st[i] for i in nonfinite])
    assert all(st[i] & ST_REJECTED for i in gated), (name, [st[i] for i in gated])
    plain = ~inactive
    plain[list(dead) + list(bad) + list(nonfinite) + list(gated)] = False
    ok = plain & (st == 0)
    assert ok.sum() > 0.9 * plain.sum() and ok[20] + ok[23] >= 1, (name, int(ok.sum()), int(plain.sum()), np.unique(st[plain]))
    for k in per_filter:
        assert np.isfinite(got[k][ok]).all(), (name, k)
    for k in per_candidate:
        assert np.isfinite(got[k][:, ok]).all(), (name, k)
    if commit is None:
        return ok
    if commit:
        assert not np.array_equal(before[0][ok], after[0][ok]) and not np.array_equal(before[1][ok], after[1][ok]), name
        assert np.isfinite(after[0][ok]).all() and np.isfinite(after[1][ok]).all(), name
    else:
        assert same_snapshot(before, after), name
    return ok


def forms(mode):
    """the read-only form in every cell, the committing one in fp64 and in the wide instantiation"""
    return (False, True) if mode != "f32" else (False,)


# -------------------------------------------------------------------------------------------- sensor frame, robust, association
def sensor_case(spe, model, mode):
    c = base(spe, model, mode)
    if not hasattr(c, "mount"):
        c.mount, c.point, gyro, c.z, c.Q = smc.make_inputs(model, c.mu, c.dtype)
        if model == "orient":
            c.in_b = gyro
        c.gyro = gyro
        ids = smc.cycling_ids(model, c.n)       # every model of the engine (m = 1 and m = 3 side by side), -1 and a foreign id
        ids[every_seventh(c.n)] = -1
        ids[[BAD, DEAD, NANZ, GATED, 20]] = sr.ids_of(man_of(model))[0]
        ids[23] = sr.ids_of(man_of(model))[-1]
        c.ids = ids
        c.idle = ~np.isin(ids, sr.ids_of(man_of(model)))
    return c


def sensor_inputs(c, z):
    return dict(z_dev=up(c, z), Q_dev=up(c, c.Q.reshape(c.n, 9)), model_dev=up(c, c.ids, torch.int32), mount_dev=up(c, c.mount),
                point_dev=up(c, c.point))


def meas_outs(c, m=3, n=None):
    n = c.n if n is None else n
    return {"z_pred": nans(c, n, m), "S": nans(c, n, m * m), "innov": nans(c, n, m), "maha": nans(c, n), "loglik": nans(c, n),
            "status": ints(n)}


@cells
def test_sensor_frame(spe, model, mode):
    c = sensor_case(spe, model, mode)
    z = smc.mixed_z(c, c.ids)
    z[NANZ, 0] = np.nan
    z[GATED] += 100.0
    i = sensor_inputs(c, z)
    for commit in forms(mode):
        o = meas_outs(c)
        name = f"sensor/{model}/{mode}/commit={commit}"
        r = leftovers(spe, c, lambda e: e.update_sensor_dev(0, i["z_dev"], i["Q_dev"], model_dev=i["model_dev"], mount_dev=i["mount_dev"],
                                                            point_dev=i["point_dev"], commit=commit, **o), o, name, gate_chi2=GATE)
        judge(c, name, *r, commit, inactive=c.idle, nonfinite=[NANZ], gated=[GATED], per_filter=("maha", "loglik"))


def spread_samples(c, factors):
    """the case's samples with their innovations scaled filter by filter: z = h + factor (z - h)"""
    z = np.zeros((c.n, 3))
    f = np.asarray(factors, dtype=np.float64)[np.arange(c.n) % len(factors)]
    for mid in sr.ids_of(man_of(c.model)):
        m, rows = sr.meas_dim(mid), c.ids == mid
        h = sr.h(mid, c.mu, c.mount, c.point, c.gyro)
        z[rows, :m] = (h + f[:, None] * (c.z[mid][:, :m] - h))[rows]
    return stored(z, c.dtype)


@cells
@pytest.mark.parametrize("rule", ["match", "huber"])
def test_robust(spe, model, mode, rule):
    """inliers, inflated rows whose Newton iterations differ in length, and gated rows in one wavefront: factors 1 ... 1000"""
    c = sensor_case(spe, model, mode)
    z = spread_samples(c, (1.0, 4.0, 12.0, 40.0, 2.0, 1000.0, 7.0, 25.0))
    z[NANZ, 0] = np.nan
    z[GATED] += 100.0
    i = sensor_inputs(c, z)
    rl = spe.RobustRule(rob.MATCH if rule == "match" else rob.HUBER, rob.CHI2_M1, rob.CHI2_M3, 1e30, 2e-6 if mode == "f32" else 1e-13, 16)
    for commit in forms(mode) if rule == "match" else (False,):
        o = meas_outs(c)
        o.update(maha0=nans(c, c.n), scale=nans(c, c.n), iterations=ints(c.n))
        name = f"robust/{rule}/{model}/{mode}/commit={commit}"
        r = leftovers(spe, c, lambda e: e.update_robust_dev(0, i["z_dev"], i["Q_dev"], rl, model_dev=i["model_dev"], mount_dev=i["mount_dev"],
                                                            point_dev=i["point_dev"], commit=commit, **o), o, name, gate_chi2=GATE)
        got = r[0]
        st = got["status"].astype(np.uint32)
        live = ~c.idle
        live[[BAD, DEAD, NANZ]] = False
        rejected = live & ((st & ST_REJECTED) != 0)
        assert rejected[GATED] and rejected.sum() > c.n // 20, (name, int(rejected.sum()))
        scored = live & (st == 0)
        inflated = scored & (got["scale"] > 1.0)
        assert inflated.sum() > c.n // 20 and (scored & (got["scale"] <= 1.0)).sum() > c.n // 20, name
        if rule == "match":
            assert len(set(got["iterations"][inflated].tolist())) > 1, name   # trip counts differ inside the batch
        # the gated rows are planted here: everything else must be 0, and finite
        judge(c, name, *r, commit, inactive=c.idle | rejected, nonfinite=[NANZ], per_filter=("maha0", "maha", "loglik", "scale"),
              st=np.where(rejected, ST_INACTIVE, st))


@cells
def test_association(spe, model, mode):
    """K = 3 candidates of one point: the true sample, one a few sigmas off, one far off; every fifth filter's second is NaN"""
    c = sensor_case(spe, model, mode)
    z0 = smc.mixed_z(c, c.ids)
    z = np.stack([z0 + 0.2, z0, z0 + 3.0])
    z[1, ::5] = np.nan
    z[:, NANZ] = np.nan
    z[:, GATED] += 100.0
    i = sensor_inputs(c, z)
    for commit in forms(mode):
        o = {"z_pred": nans(c, 1, c.n, 3), "S": nans(c, 1, c.n, 9), "innov": nans(c, 3, c.n, 3), "maha": nans(c, 3, c.n),
             "loglik": nans(c, 3, c.n), "best": ints(c.n), "n_gated": ints(c.n), "status": ints(c.n)}
        name = f"associate/{model}/{mode}/commit={commit}"
        r = leftovers(spe, c, lambda e: e.associate_sensor_dev(0, 3, i["z_dev"], i["Q_dev"], model_dev=i["model_dev"], mount_dev=i["mount_dev"],
                                                               point_dev=i["point_dev"], commit=commit, **o), o, name, gate_chi2=GATE)
        ok = judge(c, name, *r, commit, inactive=c.idle, nonfinite=[NANZ], gated=[GATED])
        best = r[0]["best"]
        assert (best[ok] >= 0).all() and len(set(best[ok].tolist())) > 1 and np.isfinite(r[0]["maha"][best[ok], np.nonzero(ok)[0]]).all(), name


# ------------------------------------------------------------------------------------------------------------------ bearing
@cells
def test_bearing(spe, model, mode):
    c = base(spe, model, mode)
    man = man_of(model)
    mount, point, zs, Q = bear.make_inputs(man, c.mu, 15.0, 80.0, c.dtype)
    table = list(bear.ids_of(man)) + [-1]
    ids = np.array(table, dtype=np.int32)[np.arange(c.n) % len(table)]
    ids[every_seventh(c.n)] = -1
    ids[[BAD, DEAD, NANZ, GATED, GATED + 1, 20]] = bear.ids_of(man)[0]
    ids[23] = bear.ids_of(man)[-1]
    z = np.ones((c.n, 3))
    for mid in bear.ids_of(man):
        z[ids == mid] = zs[mid][ids == mid]
    z[NANZ, 1] = np.nan
    z[GATED] = np.cross(z[GATED], [0.3, -0.5, 0.8])   # a quarter turn away: d^2 of about (pi / 2)^2 / 0.05^2 = 1e3
    z[GATED + 1] = -z[GATED + 1]                      # next to the antipode of the predicted direction
    idle = ids < 0
    zd, qd, idd, md, pd = up(c, z), up(c, Q.reshape(c.n, 9)), up(c, ids, torch.int32), up(c, mount), up(c, point)
    for commit in forms(mode):
        o = meas_outs(c)
        name = f"bearing/{model}/{mode}/commit={commit}"
        r = leftovers(spe, c, lambda e: e.update_bearing_dev(0, zd, qd, model_dev=idd, mount_dev=md, point_dev=pd, commit=commit, **o), o,
                      name, gate_chi2=BEARING_GATE)
        assert r[0]["status"][GATED + 1] != 0, name
        judge(c, name, *r, commit, inactive=idle, nonfinite=[NANZ], gated=[GATED, GATED + 1], per_filter=("z_pred", "S", "maha", "loglik"),
              st=np.where(np.arange(c.n) == GATED + 1, ST_REJECTED, r[0]["status"].astype(np.uint32)))


# ------------------------------------------------------------------------------------------------------------- state blocks
@cells
def test_state_blocks(spe, model, mode):
    """a mask per filter that runs through every block set of the model, the orientation block alone and in company included"""
    c = base(spe, model, mode)
    z, Qz = smr.make_inputs(man_of(model), c.mu, c.cov, c.dtype)
    masks = smr.cycling_masks(model, c.n)
    masks[every_seventh(c.n)] = 0
    masks[[BAD, DEAD, NANZ, GATED]] = smr.full_mask(model)
    velocity = slice(7, 10) if model == "pose" else slice(4, 7)
    z[NANZ, velocity] = np.nan
    z[GATED, velocity] += 100.0
    zd, qd, md = up(c, z), up(c, pack(Qz)), up(c, masks, torch.int32)
    for commit in forms(mode):
        o = {"maha": nans(c, c.n), "loglik": nans(c, c.n), "status": ints(c.n)}
        name = f"state/{model}/{mode}/commit={commit}"
        r = leftovers(spe, c, lambda e: e.update_state_dev(0, zd, qd, block_mask_dev=md, commit=commit, **o), o, name, gate_chi2=GATE)
        judge(c, name, *r, commit, inactive=masks == 0, nonfinite=[NANZ], gated=[GATED], per_filter=("maha", "loglik"))


# ---------------------------------------------------------------------------------------------------------------- innovation
@cells
def test_innovation_and_selection(spe, model, mode):
    """K = 3 candidates; Pose: a model per filter over the nine, the linear selections and the SO(3) sigma-point model side by
    side, a quarter of the filters without one; OrientationState has the one (sigma-point) model"""
    c = base(spe, model, mode)
    sy = spe.synth
    rng = np.random.default_rng(3)
    if model == "pose":
        models = sy.pose_mixed_models(c.n, 0)
        models[[BAD, DEAD, NANZ, GATED]] = spe.MEAS_POS3
        models[20], models[23] = spe.MEAS_ORIENT_SO3, spe.MEAS_VEL_XY
        z = np.stack([sy.pose_measurement_for_model(c.mu, models, s * rng.standard_normal((c.n, 3))) for s in (0.3, 0.05, 1.0)])
    else:
        models = np.where(every_seventh(c.n), -1, spe.MEAS_ORIENT_BODYVEL3).astype(np.int32)
        z0 = sy.orient_cycle_inputs(c.n, 2, c.mu[:, 0:4])[2]
        z = np.stack([z0 + s * rng.standard_normal((c.n, 3)) for s in (0.3, 0.0, 1.0)])
    z[:, NANZ] = np.nan
    z[:, GATED] += 1000.0
    z = stored(z, c.dtype)
    zd, qd, md = up(c, z), up(c, 0.05 ** 2 * np.eye(3).reshape(9)), up(c, models, torch.int32)
    o = {"z_pred": nans(c, c.n, 4), "S": nans(c, c.n, 9), "innov": nans(c, 3, c.n, 3), "maha": nans(c, 3, c.n), "loglik": nans(c, 3, c.n),
         "best": ints(c.n), "status": ints(c.n)}
    name = f"innovation/{model}/{mode}"
    r = leftovers(spe, c, lambda e: e.innovation_dev(0, 3, zd, qd, q_is_uniform=True, meas_model_dev=md, **o), o, name, gate_chi2=GATE)
    got = r[0]
    st = got["status"].astype(np.uint32)
    assert got["best"][GATED] == -1 and st[NANZ] != 0, (name, got["best"][GATED], st[NANZ])
    odd = np.isin(np.arange(c.n), (NANZ, GATED))   # judged above
    ok = judge(c, name, *r, False, inactive=(models < 0) | odd, per_filter=("S",), per_candidate=("maha", "loglik"),
               st=np.where(odd, ST_INACTIVE, st))
    assert (got["best"][ok] >= 0).sum() > ok.sum() // 2, name
    # the selection that follows it, from the winners of the run above
    best = up(c, got["best"], torch.int32)
    o2 = {"z_sel": nans(c, c.n, 3), "model_sel": ints(c.n)}
    name = f"select/{model}/{mode}"
    r = leftovers(spe, c, lambda e: e.select_candidates_dev(3, best, 0, zd, o2["z_sel"], o2["model_sel"], meas_model_dev=md), o2, name)
    assert same_snapshot(r[1], r[2]), name
    won = got["best"] >= 0
    assert np.array_equal(r[0]["model_sel"], np.where(won, models, -1)), name
    assert np.array_equal(r[0]["z_sel"][won], up(c, z).cpu().numpy()[got["best"][won], np.nonzero(won)[0]]), name


# ------------------------------------------------------------------------------------------------- user-defined models
def exported(spe, c):
    """the sigma points of the planted engine (NaN rows for DEAD and BAD), made once per case"""
    if not hasattr(c, "X"):
        e = planted(spe, c)
        c.X = nans(c, c.n, 2 * c.D + 1, c.S)
        e.sigma_points_dev(c.X, None, None)
        e.sync()
        torch.cuda.synchronize()
        e.close()
    return c.X


@cells
def test_sampled_update(spe, model, mode):
    """sigma_points_dev, then update_sampled_dev on samples of a one- and a six-dimensional user model"""
    c = base(spe, model, mode)
    o = {"X": nans(c, c.n, 2 * c.D + 1, c.S), "delta": nans(c, c.n, 2 * c.D + 1, c.D), "status": ints(c.n)}
    name = f"sigma_points/{model}/{mode}"
    r = leftovers(spe, c, lambda e: e.sigma_points_dev(o["X"], o["delta"], o["status"]), o, name)
    judge(c, name, *r, False, per_filter=("X", "delta"))
    X = exported(spe, c)
    assert np.array_equal(X.cpu().numpy(), r[0]["X"], equal_nan=True), name
    active = (~every_seventh(c.n)).astype(np.uint8)
    rng = np.random.default_rng(7)
    six = [0, 1, 2, 7, 8, 9] if model == "pose" else [4, 5, 6, 7, 8, 9]   # position and velocity / velocity and gyro bias
    for m, comps in ((1, six[:1]), (6, six)):
        Z = X[:, :, comps].contiguous()
        z = np.nan_to_num(Z[:, 0, :].double().cpu().numpy()) + 0.05 * rng.standard_normal((c.n, m))
        z[NANZ, 0] = np.nan
        z[GATED] += 100.0
        zd, qd, ad = up(c, z), up(c, np.broadcast_to(0.05 ** 2 * np.eye(m), (c.n, m, m))), up(c, active, torch.uint8)
        for commit in forms(mode):
            om = meas_outs(c, m)
            name = f"sampled/m={m}/{model}/{mode}/commit={commit}"
            r = leftovers(spe, c, lambda e: e.update_sampled_dev(m, Z, zd, qd, active_dev=ad, commit=commit, **om), om, name, gate_chi2=GATE)
            judge(c, name, *r, commit, inactive=active == 0, nonfinite=[NANZ], gated=[GATED], per_filter=("z_pred", "S", "maha", "loglik"))


@cells
def test_sampled_predict(spe, model, mode):
    """predict_sampled_dev on the exported points themselves (f = identity) with a noise matrix per filter, and with one"""
    c = base(spe, model, mode)
    XX = exported(spe, c)
    active = (~every_seventh(c.n)).astype(np.uint8)
    ad = up(c, active, torch.uint8)
    rng = np.random.default_rng(9)
    A = 0.01 * rng.standard_normal((c.n, c.D, c.D))
    R = 1e-4 * np.eye(c.D) + A @ np.swapaxes(A, 1, 2)
    for uniform, Rd in ((False, up(c, R)), (True, up(c, R[0]))):
        for commit in forms(mode) if not uniform else (False,):
            o = {"mu": nans(c, c.n, c.S), "cov_packed": nans(c, c.n, c.PK), "status": ints(c.n)}
            name = f"predict_sampled/uniform={uniform}/{model}/{mode}/commit={commit}"
            r = leftovers(spe, c, lambda e: e.predict_sampled_dev(XX, Rd, r_is_uniform=uniform, active_dev=ad, commit=commit, **o), o, name)
            judge(c, name, *r, None, inactive=active == 0, per_filter=("mu", "cov_packed"))
            ok = (r[0]["status"] == 0)
            if commit:   # the mean is the points' own (f = identity): the covariance is what moves
                assert not np.array_equal(r[1][1][ok], r[2][1][ok]) and np.isfinite(r[2][1][ok]).all(), name
            else:
                assert same_snapshot(r[1], r[2]), name


# ------------------------------------------------------------------------------------------------------------------ forecast
@cells
def test_forecast(spe, model, mode):
    """five steps into a ring of eight from slot 5 (slots 5, 6, 7, 0, 1): from the engine's state with input rings, and from a
    start record with the latched inputs"""
    c = base(spe, model, mode)
    sy = spe.synth
    in_a, in_b = torch.zeros((SLOTS, c.n, 3), dtype=c.T, device="cuda"), torch.zeros((SLOTS, c.n, 3), dtype=c.T, device="cuda")
    for k in range(5):
        if model == "pose":
            a, b = sy.pose_cycle_inputs(c.n, 3 + k, c.mu[:, :3])[0], np.zeros((c.n, 3))
            a[k::5] = np.nan   # the constant-velocity branch
        else:
            b, a = sy.orient_cycle_inputs(c.n, 3 + k, c.mu[:, 0:4])[:2]
        in_a[(FIRST + k) % SLOTS], in_b[(FIRST + k) % SLOTS] = up(c, a), up(c, b)
    dt = [0.01, 0.011, 0.012, 0.013, 0.014]
    cov = c.cov.copy()
    cov[BAD, 2, 1] = cov[BAD, 1, 2] = np.nan
    start = (up(c, c.mu), up(c, pack(cov)))
    for given in (False, True):
        o = {"mu": nans(c, SLOTS, c.n, c.S), "cov": nans(c, SLOTS, c.n, c.PK), "status": ints(c.n)}
        name = f"forecast/start={given}/{model}/{mode}"
        if given:
            call = lambda e: e.forecast_dev(SLOTS, FIRST, o["mu"], o["cov"], o["status"], dt=dt, start_mu=start[0], start_cov=start[1])   # noqa: E731
        else:
            call = lambda e: e.forecast_dev(SLOTS, FIRST, o["mu"], o["cov"], o["status"], dt=dt, in_a_dev=in_a, in_b_dev=in_b)   # noqa: E731
        r = leftovers(spe, c, call, o, name)
        ok = judge(c, name, *r, False)
        written = [(FIRST + k) % SLOTS for k in range(5)]
        assert np.isfinite(r[0]["mu"][written][:, ok]).all() and np.isfinite(r[0]["cov"][written][:, ok]).all(), name
        assert np.isnan(r[0]["mu"][[2, 3, 4]]).all(), name   # the slots outside the window keep the sentinel


# ------------------------------------------------------------------------------------------ the history: smoother, late samples
_REC = {}


def recorded(spe, model, mode):
    """six steps of real cycles, every filtered state pushed into a ring of eight from slot 5 with history_push_dev -> the case
    of the engine at the last step, the rings (filter BAD's covariance at step 3 indefinite, in the caller's ring) and the inputs"""
    key = (model, mode)
    if key in _REC:
        return _REC[key]
    sy = spe.synth
    c0 = base(spe, model, mode)
    e = planted(spe, c0)
    e.initialize(c0.mu[BAD:BAD + 1], c0.cov[BAD:BAD + 1], first=BAD)   # the recording is healthy but for DEAD
    mu_hist, cov_hist = torch.zeros((SLOTS, N, c0.S), dtype=c0.T, device="cuda"), torch.zeros((SLOTS, N, c0.PK), dtype=c0.T, device="cuda")
    in_a, in_b = torch.zeros((SLOTS, N, 3), dtype=c0.T, device="cuda"), torch.zeros((SLOTS, N, 3), dtype=c0.T, device="cuda")
    dt = np.array([0.01 * (1.0 + 0.1 * k) for k in range(STEPS - 1)])
    for k in range(STEPS):
        slot = (FIRST + k) % SLOTS
        mu_now = np.where((np.arange(N) == DEAD)[:, None], c0.mu, e.state(with_cov=False)[0])
        if model == "pose":
            a, z, Q = sy.pose_cycle_inputs(N, 3 + k, mu_now[:, :3])
            a[k::5] = np.nan   # the constant-velocity branch
            b = np.zeros((N, 3))
        else:
            b, a, z, Q = sy.orient_cycle_inputs(N, 3 + k, mu_now[:, 0:4])
        if k > 0:
            e.cycle(float(dt[k - 1]), spe.MEAS_POS3 if model == "pose" else spe.MEAS_ORIENT_BODYVEL3, z, Q)
        e.history_push_dev(SLOTS, slot, mu_hist, cov_hist)
        # the inputs of the prediction k -> k + 1: latched now, and into the ring at step k's slot
        if model == "pose":
            e.set_acceleration(a, ACC_COV)
        else:
            e.set_orient_inputs(b, a)
        in_a[slot], in_b[slot] = up(c0, a), up(c0, b)
    e.sync()
    torch.cuda.synchronize()
    c = Case()
    c.__dict__.update({k: v for k, v in c0.__dict__.items() if k not in ("X", "mount")})
    c.mu, c.cov, init = e.state()
    assert not init[DEAD] and init.sum() == N - 1
    c.mu[DEAD], c.cov[DEAD] = c0.mu[DEAD], c0.cov[DEAD]
    c.in_a, c.in_b = np.nan_to_num(a, nan=0.1), b
    c.bad = N - 1        # the engine's own failing filter: the last workgroup's only one
    e.close()
    bad_slot = (FIRST + 3) % SLOTS
    cov_hist[bad_slot, BAD] = up(c0, -np.eye(c0.D)[np.tril_indices(c0.D)])
    c.mu_hist, c.cov_hist, c.ring_a, c.ring_b, c.dt = mu_hist, cov_hist, in_a, in_b, dt
    c.mu_host = mu_hist.double().cpu().numpy()
    _REC[key] = c
    return c


@cells
def test_smoother(spe, model, mode):
    """smooth_dev over the wrapped window: input rings and a covariance output; the latched inputs and none"""
    c = recorded(spe, model, mode)
    for rings, want_cov in ((True, True), (False, False)):
        o = {"mu": nans(c, SLOTS, N, c.S), "status": ints(N)}
        if want_cov:
            o["cov"] = nans(c, SLOTS, N, c.PK)
        name = f"smooth/rings={rings}/cov={want_cov}/{model}/{mode}"
        r = leftovers(spe, c, lambda e: e.smooth_dev(c.dt, SLOTS, FIRST, c.mu_hist, c.cov_hist, o["mu"], o.get("cov", False), o["status"],
                                                     in_a_dev=c.ring_a if rings else None, in_b_dev=c.ring_b if rings else None), o, name)
        # the engine's own covariance is not read: its failing filter N - 1 smooths like any other; BAD fails in the ring
        ok = judge(c, name, *r, False, bad=[BAD])
        window = [(FIRST + k) % SLOTS for k in range(STEPS)]
        assert np.isfinite(r[0]["mu"][window][:, ok]).all() and (not want_cov or np.isfinite(r[0]["cov"][window][:, ok]).all()), name
        assert not np.array_equal(r[0]["mu"][window[0]][ok], c.mu_hist[window[0]].cpu().numpy()[ok]), name


def late_inputs(spe, c, model):
    """lags 0 ... 5 spread over the filters, a model id per filter (-1 on every seventh), samples near each filter's own step"""
    lag = (np.arange(N) % STEPS).astype(np.int32)
    lag[[BAD, GATED, NANZ]] = 2, 3, 1     # BAD: the indefinite record of step 3
    rng = np.random.default_rng(13)
    full = spe.MEAS_POS3 if model == "pose" else spe.MEAS_ORIENT_BODYVEL3
    models = np.where(every_seventh(N), -1, full).astype(np.int32)
    if model == "pose":
        at = np.where((lag > 0)[:, None], c.mu_host[(FIRST + STEPS - 1 - lag) % SLOTS, np.arange(N)], c.mu)
        z = at[:, 0:3] + 0.05 * rng.standard_normal((N, 3))
    else:
        z = 0.05 * rng.standard_normal((N, 3))
    z[NANZ, 2] = np.nan
    z[GATED] += 100.0
    return lag, models, stored(z, c.dtype)


@cells
def test_late_samples(spe, model, mode):
    c = recorded(spe, model, mode)
    lag, models, z = late_inputs(spe, c, model)
    ld, md, zd, qd = up(c, lag, torch.int32), up(c, models, torch.int32), up(c, z), up(c, 0.05 ** 2 * np.eye(3).reshape(9))
    for commit in forms(mode):
        o = {"z_pred": nans(c, N, 4), "S": nans(c, N, 9), "innov": nans(c, N, 3), "maha": nans(c, N), "loglik": nans(c, N),
             "status": ints(N), "mu_out": nans(c, N, c.S), "cov_out": nans(c, N, c.PK)}
        name = f"delayed/{model}/{mode}/commit={commit}"
        r = leftovers(spe, c, lambda e: e.update_delayed_dev(c.dt, SLOTS, FIRST, c.mu_hist, c.cov_hist, ld, md, zd, qd, q_is_uniform=True,
                                                             in_a_dev=c.ring_a, in_b_dev=c.ring_b, commit=commit, **o), o, name, gate_chi2=GATE)
        judge(c, name, *r, commit, inactive=models < 0, nonfinite=[NANZ], gated=[GATED], bad=[BAD, c.bad],
              per_filter=("S", "maha", "loglik", "mu_out", "cov_out"))


# Relative measurements are a PoseWithVelocity feature: an OrientationState engine refuses the call (tests/test_gpu_relative.py),
# so the orient cells are left out.
@pytest.mark.parametrize("mode", list(MODES))
def test_relative(spe, mode):
    """the three relative models side by side, lags 0 (refused) ... 5 spread over the filters"""
    c = recorded(spe, "pose", mode)
    lag = (np.arange(N) % STEPS).astype(np.int32)
    lag[[BAD, GATED, NANZ, N - 1]] = 2, 3, 1, 1   # BAD: the indefinite record of step 3; N - 1: the engine's own failing filter
    then = c.mu_host[(FIRST + STEPS - 1 - lag) % SLOTS, np.arange(N)].copy()
    then[DEAD] = c.mu[DEAD]
    models, z, Q = rc.increments(spe, N, c.mu, then)
    z[NANZ] = np.nan
    z[GATED, 0:3] = 100.0
    models[GATED] = rc.rr.POSITION
    z = stored(z, c.dtype)
    idle = (lag == 0) | every_seventh(N)
    per = np.where(every_seventh(N), -1, models).astype(np.int32)
    ld, md, zd, qd = up(c, lag, torch.int32), up(c, per, torch.int32), up(c, z), up(c, Q.reshape(36))
    for commit in forms(mode):
        o = {"z_pred": nans(c, N, 7), "S": nans(c, N, 36), "innov": nans(c, N, 6), "maha": nans(c, N), "loglik": nans(c, N),
             "status": ints(N), "mu_out": nans(c, N, c.S), "cov_out": nans(c, N, c.PK)}
        name = f"relative/{mode}/commit={commit}"
        r = leftovers(spe, c, lambda e: e.update_relative_dev(c.dt, SLOTS, FIRST, c.mu_hist, c.cov_hist, ld, md, zd, qd, q_is_uniform=True,
                                                              in_a_dev=c.ring_a, commit=commit, **o), o, name, gate_chi2=GATE)
        judge(c, name, *r, commit, inactive=idle, nonfinite=[NANZ], gated=[GATED], bad=[BAD, c.bad], per_filter=("maha", "loglik", "mu_out", "cov_out"))


# --------------------------------------------------------------------------------------------------------------------- banks
@cells
@pytest.mark.parametrize("M,T", [(3, 85), (8, 31)])
def test_bank(spe, model, mode, M, T):
    """85 tracks of 3 hypotheses on 255 filters (the last workgroup holds one track) and 31 of 8 on 248: weights, mixture moments
    and the IMM interaction; track 5 holds the uninitialised filter and track 6 the failing one, 4 and 7 are healthy wave-mates"""
    man, mu, cov, w = br.make_tracks(spe, on, model, T, M)
    c = base(spe, model, mode, T * M, state=(mu.reshape(T * M, man.S), cov.reshape(T * M, man.D, man.D)))
    c.dead, c.bad = 5 * M + 1, 6 * M
    w = stored(w, c.dtype)
    rng = np.random.default_rng(5)
    ll = rng.uniform(-30.0, 5.0, (T, M))
    ll[::7] -= 690.0
    ll[3::11, 2] = np.nan      # a dead hypothesis
    ll[9] = np.nan             # every hypothesis of a track dead
    lw_d, ll_d, w_d = up(c, stored(np.log(w), c.dtype).reshape(-1)), up(c, stored(ll, c.dtype).reshape(-1)), up(c, w.reshape(-1))
    tracks = np.ones(T, bool)
    tracks[[5, 6]] = False
    o = {"logw": nans(c, T * M), "w": nans(c, T * M), "status": ints(T)}
    name = f"bank_weights/M={M}/{model}/{mode}"
    r = leftovers(spe, c, lambda e: e.bank_weights_dev(M, lw_d, ll_d, o["logw"], o["w"], o["status"]), o, name)
    st = r[0]["status"].astype(np.uint32)
    assert same_snapshot(r[1], r[2]) and st[9] == ST_WEIGHTS and (st[np.arange(T) != 9] == 0).all(), (name, np.unique(st))
    assert np.isfinite(r[0]["w"].reshape(T, M)[st == 0]).all(), name
    o = {"mu": nans(c, T, c.S), "cov": nans(c, T, c.PK), "status": ints(T)}
    name = f"bank_combine/M={M}/{model}/{mode}"
    r = leftovers(spe, c, lambda e: e.bank_combine_dev(M, w_d, o["mu"], o["cov"], o["status"]), o, name)
    st = r[0]["status"].astype(np.uint32)
    assert same_snapshot(r[1], r[2]) and st[5] != 0 and (st[tracks] == 0).sum() > 0.9 * tracks.sum() and st[4] == 0 and st[7] == 0, (name, st)
    assert np.isfinite(r[0]["mu"][tracks & (st == 0)]).all() and np.isfinite(r[0]["cov"][tracks & (st == 0)]).all(), name
    P = br.transition(M)
    o = {"w_pred": nans(c, T * M), "status": ints(T)}
    name = f"bank_mix/M={M}/{model}/{mode}"
    r = leftovers(spe, c, lambda e: e.bank_mix_dev(M, w_d, P, o["w_pred"], o["status"]), o, name)
    st = r[0]["status"].astype(np.uint32)
    assert st[5] != 0 and (st[tracks] == 0).sum() > 0.9 * tracks.sum() and st[4] == 0 and st[7] == 0, (name, st)
    moved = np.repeat(tracks & (st == 0), M)
    assert not np.array_equal(r[1][0][moved], r[2][0][moved]) and np.isfinite(r[2][0][moved]).all() and np.isfinite(r[2][1][moved]).all(), name
    assert np.isfinite(r[0]["w_pred"][moved]).all(), name


# ----------------------------------------------------------------------------------------------------------------- lifecycle
@cells
@pytest.mark.parametrize("group,n", [(1, 253), (4, 252)])   # a group must divide the capacity: 252 = 63 x 4
def test_compaction(spe, model, mode, group, n):
    """retire_dev with a ragged mask, then compact_dev (the hipcub scans of ukf_lifecycle.hpp); the poison goes in front of both"""
    c = base(spe, model, mode, n)
    rng = np.random.default_rng(21)
    mask = (rng.random(n) < 0.4).astype(np.uint8)
    mask[[20, 23]] = 0
    md = up(c, mask, torch.uint8)
    name = f"retire/{model}/{mode}/n={n}"
    r = leftovers(spe, c, lambda e: e.retire_dev(md), {}, name)
    assert np.array_equal(r[2][2], r[1][2] & (mask == 0)) and r[2][2].sum() < r[1][2].sum(), name
    o = {"new_index": ints(n), "old_index": ints(n), "live": ints(1, dtype=torch.int64)}
    name = f"compact/{model}/{mode}/group={group}"
    got, before, after = leftovers(spe, c, lambda e: e.compact_dev(group, o["new_index"], o["old_index"], o["live"]), o, name,
                                   prepare=lambda e: e.retire_dev(md))
    alive = (mask == 0) & (np.arange(n) != DEAD)
    groups = alive.reshape(-1, group).any(axis=1)
    assert int(got["live"][0]) == int(groups.sum()) * group and 0 < groups.sum() < groups.size, (name, got["live"], int(groups.sum()))
    assert after[2][:int(got["live"][0])].any() and not after[2][int(got["live"][0]):].any(), name
    assert np.array_equal(np.sort(got["old_index"][:int(got["live"][0])]), np.nonzero(np.repeat(groups, group))[0]), name

