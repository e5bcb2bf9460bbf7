"""Filter lifecycle on the device (ukfb_gather_filters_dev / ukfb_scatter_filters_dev / ukfb_retire_dev / ukfb_compact_dev and the
host forms, include/ukf_batch.h "filter lifecycle").

Every call moves bits and computes nothing (the one product, the 2 acc.cov block of a Pose filter's acceleration-branch noise, is
build_racc_kernel's expression), so every comparison is BIT FOR BIT against tests/lifecycle_reference.py (pinned by
tests/test_lifecycle_reference.py) unless it says otherwise.  The engines are cycled three times first, two of the cycles with
per-filter timestamps, so that states, status words and last measurement times differ from filter to filter.

How the engine is read back: mean, covariance and status words by a plain device-to-host copy through the pointers of
ukfb_device_views, flags and times by their getters.  The latches and the per-filter noise have no getter that returns their
bits for every filter at once; test_gather holds the gather against the values the setters were given (and against
ukfb_get_process_noise), and the other tests then read those fields with a gather of every filter.  The acceleration-branch
noise of a Pose filter cannot be read at all: it is checked through behaviour, a cycle on the acceleration branch
(test_round_trip_is_complete, test_compact_then_run).

test_compact_then_run is the one comparison with a tolerance: a filter that moves gets other wave-mates, and the header promises
agreement to rounding then -- the suite's fp64 parity bound 1e-9 (1 + |ref|).  It prints the measured maximum (a PARITY line;
profiles/lifecycle_parity.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lifecycle_reference as lr
from engine_support import ACC_COV, new_engine, same_snapshot, snapshot, tdt

pytestmark = pytest.mark.gpu

N = 1022   # not a multiple of four: the last workgroup holds two filters
PRECS = [("f64", 0), ("f32", 1)]
IDS = [p[0] for p in PRECS]
MODELS = ["pose", "orient"]
ST_UNINITIALISED, ST_INACTIVE = 1 << 7, 1 << 8
_HIP = None


def raw(ptr, shape, dtype):
    """a device array as it lies, by hipMemcpy (the engine has been synchronised by the caller)"""
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
    out = np.empty(shape, dtype=dtype)
    assert _HIP.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def to_dev(x, dtype=None):
    """x on the device in its own dtype (integer indices and masks stay integers), or in `dtype`"""
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype) if dtype is not None else torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def to_host(t):
    """a device tensor on the host in its own dtype"""
    return t.cpu().numpy()


class Rig:
    """a cycled engine and what the setters were given last (in the engine's storage type)"""


def inputs(spe, model, n, c, mu_now, first=0):
    sy = spe.synth
    if model == "pose":
        acc, z, Q = sy.pose_cycle_inputs(n, c, mu_now[:, :3], first=first)
        return acc, np.zeros((n, 3)), z, Q
    gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu_now[:, 0:4], first=first)
    return acc, gyro, z, Q


def latch(r, a, b):
    if r.model == "pose":
        r.e.set_acceleration(a, ACC_COV)
    else:
        r.e.set_orient_inputs(b, a)
    r.latch_a, r.latch_b = a.astype(r.e.dtype), b.astype(r.e.dtype)


def stamps(n, k):
    i = np.arange(n, dtype=np.int64)
    # every fifth filter keeps its first stamp: its later samples come with dt = 0, so the status words differ between filters
    return 1_000_000 + 1000 * i + k * (10_000 + 100 * (i % 7)) * (i % 5 != 0)


def make(spe, model, n, prec, per_filter_noise=False, first=0, skip=(), cycles=True):
    """first: which filters of synth's population the engine holds (two rigs with different `first` hold different filters)"""
    sy = spe.synth
    r = Rig()
    r.e, r.model, r.n = new_engine(spe, model, n, prec, 0), model, n
    e = r.e
    r.per_filter_noise = per_filter_noise
    if per_filter_noise:   # every filter its own matrix
        scale = 1.0 + np.arange(n) / n + 0.5 * (np.arange(n) % 3 == 0)
        e.set_process_noise(scale[:, None, None] * e.process_noise()[None])
    mu0, cov0 = sy.pose_initial(n, first=first) if model == "pose" else sy.orient_initial(n, first=first)
    if skip:   # filters [skip[0], skip[1]) stay uninitialised
        if skip[0] > 0:
            e.initialize(mu0[:skip[0]], cov0[:skip[0]])
        if skip[1] < n:
            e.initialize(mu0[skip[1]:], cov0[skip[1]:], first=skip[1])
    else:
        e.initialize(mu0, cov0)
    r.meas = spe.MEAS_POS3 if model == "pose" else spe.MEAS_ORIENT_BODYVEL3
    r.first = first
    if model == "pose":
        e.set_acceleration(None, ACC_COV)
    r.latch_a = r.latch_b = None
    for c in range(3 if cycles else 0):
        cycle(spe, r, c)
    return r


def cycle(spe, r, c, stamped=None):
    """cycle c of the rig: 0 and 2 with per-filter timestamps (0 only latches the times), 1 with one time step"""
    e, n = r.e, r.n
    a, b, z, Q = inputs(spe, r.model, n, c, e.state(with_cov=False)[0], first=r.first)
    latch(r, a, b)
    if (c != 1) if stamped is None else stamped:
        e.cycle_timestamps(stamps(n, c // 2 if c < 3 else c), np.full(n, r.meas, dtype=np.int32), z, Q)
    else:
        e.cycle(0.01, r.meas, z, Q)


def full_gather(r, fields=("in_a", "in_b", "noise")):
    e, n = r.e, r.n
    t = tdt(e)
    out = {"in_a": torch.empty((n, 3), dtype=t, device="cuda"), "in_b": torch.empty((n, 3), dtype=t, device="cuda"),
           "noise": torch.empty((n, e.D, e.D), dtype=t, device="cuda")}
    e.gather_filters_dev(None, **{k: out[k] for k in fields})
    e.sync()
    return {k: to_host(out[k]) for k in fields}


def download(r):
    """the engine as the dict of tests/lifecycle_reference.py"""
    e, n = r.e, r.n
    e.sync()
    mu_p, cov_p, st_p = e.device_views()
    g = full_gather(r)
    s = {"mu": raw(mu_p, (n, e.S), e.dtype), "cov": raw(cov_p, (n, e.PK), e.dtype), "status": raw(st_p, (n,), np.uint32),
         "init": e.state(with_cov=False)[1].astype(np.uint8), "last_ts": e.last_measurement_time(), "in_a": g["in_a"], "in_b": g["in_b"]}
    if r.per_filter_noise:
        s["noise"] = g["noise"]
    else:   # the gather gives every filter the uniform matrix
        assert (g["noise"] == g["noise"][0]).all()
        s["noise"] = g["noise"][0].copy()
    return s


def same_state(a, b, keys=None):
    bad = [k for k in (keys or a.keys()) if not np.array_equal(a[k], b[k], equal_nan=True)]
    assert not bad, bad


def item_list(n_items, capacity, seed):
    """odd and even filter indices, duplicates (some of them threefold), -1, `capacity` and two more beyond, shuffled"""
    rng = np.random.default_rng(seed)
    base = rng.choice(capacity, size=n_items - 60, replace=False)
    dup = np.concatenate([base[:20], base[:20], base[20:30]])   # base[:20] three times in all, base[20:30] twice
    idx = np.concatenate([base, dup, [-1, -1, capacity, capacity, capacity + 5, -2 ** 31, 2 ** 31 - 1, 0, capacity - 1, capacity - 1]])
    assert idx.size == n_items and (base % 2 == 0).any() and (base % 2 == 1).any()
    return rng.permutation(idx).astype(np.int32)


def record_buffers(e, n, fill=7):
    t = tdt(e)
    return {"mu": torch.full((n, e.S), fill, dtype=t, device="cuda"), "cov_packed": torch.full((n, e.PK), fill, dtype=t, device="cuda"),
            "last_ts_us": torch.full((n,), fill, dtype=torch.int64, device="cuda"),
            "initialised": torch.full((n,), fill, dtype=torch.uint8, device="cuda"),
            "in_a": torch.full((n, 3), fill, dtype=t, device="cuda"), "in_b": torch.full((n, 3), fill, dtype=t, device="cuda"),
            "noise": torch.full((n, e.D, e.D), fill, dtype=t, device="cuda"), "status": torch.full((n,), fill, dtype=torch.int32, device="cuda")}


NAMES = {"mu": "mu", "cov_packed": "cov", "last_ts_us": "last_ts", "initialised": "init", "in_a": "in_a", "in_b": "in_b", "noise": "noise"}


@pytest.mark.parametrize("variant", ["bound", "noise"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pname,prec", PRECS, ids=IDS)
def test_gather(spe, model, pname, prec, variant):
    r = make(spe, model, N, prec, per_filter_noise=variant == "noise", skip=(500, 503))
    e = r.e
    bound_a = bound_b = None
    if variant == "bound":
        rng = np.random.default_rng(3)
        bound_a = to_dev(rng.normal(size=(N, 3)), tdt(e))
        if model == "pose":
            e.bind_acceleration_dev(bound_a)
        else:
            bound_b = to_dev(rng.normal(size=(N, 3)), tdt(e))
            e.bind_orient_inputs_dev(bound_b, bound_a)
    before = snapshot(e)
    mu_p, cov_p, _ = e.device_views()
    # the engine, read without the gather: the latches are what the setters were given (Pose engines have no in_b input: zeros)
    known = {"mu": raw(mu_p, (N, e.S), e.dtype), "cov": raw(cov_p, (N, e.PK), e.dtype), "init": before[2].astype(np.uint8),
             "last_ts": before[4], "in_a": r.latch_a, "in_b": r.latch_b, "noise": before[5].astype(e.dtype)}
    assert len(set(known["last_ts"].tolist())) > N // 2 and not known["init"][500:503].any() and known["init"].sum() == N - 3
    idx = item_list(257, N, seed=11)
    out = record_buffers(e, idx.size)
    e.gather_filters_dev(to_dev(idx), **out)
    e.sync()
    ref = lr.gather(known, idx, in_a_read=to_host(bound_a) if bound_a is not None else None,
                    in_b_read=to_host(bound_b) if bound_b is not None else None)
    for field, key in NAMES.items():
        assert np.array_equal(to_host(out[field]), ref[key], equal_nan=True), field
    assert np.array_equal(to_host(out["status"]).astype(np.uint32), ref["status"])
    assert (ref["status"] == ST_INACTIVE).sum() == 7 and not to_host(out["mu"])[ref["status"] != 0].any()
    # NULL fields are skipped; a NULL index means item k is filter k
    only = record_buffers(e, N)
    e.gather_filters_dev(None, mu=only["mu"], initialised=only["initialised"])
    e.sync()
    assert np.array_equal(to_host(only["mu"]), known["mu"]) and np.array_equal(to_host(only["initialised"]), known["init"])
    assert (to_host(only["cov_packed"]) == 7).all() and (to_host(only["status"]) == 7).all()
    assert same_snapshot(before, snapshot(e))
    e.close()


def records_from(spe, model, prec, n_items, seed):
    """n_items records of the storage type of `prec`, gathered from a cycled engine that holds other filters than the targets"""
    src = make(spe, model, N, prec, per_filter_noise=True, first=4096)
    out = record_buffers(src.e, n_items)
    src.e.gather_filters_dev(to_dev(np.random.default_rng(seed).choice(N, size=n_items, replace=False).astype(np.int32)), **out)
    src.e.sync()
    assert not to_host(out["status"]).any() and to_host(out["initialised"]).all()
    out["initialised"][::5] = 0   # every fifth record retires its filter
    out["initialised"][1::5] = 3  # any non-zero byte is "initialised"
    src.e.close()
    return out


def numpy_records(out, with_noise=True):
    rec = {key: to_host(out[field]) for field, key in NAMES.items()}
    if not with_noise:
        rec["noise"] = None
    return rec


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pname,prec", PRECS, ids=IDS)
def test_scatter(spe, model, pname, prec):
    r = make(spe, model, N, prec, per_filter_noise=True)
    e = r.e
    idx = item_list(257, N, seed=12)
    rec = records_from(spe, model, prec, idx.size, seed=13)
    before = download(r)
    views = e.device_views()
    e.scatter_filters_dev(to_dev(idx), **rec)
    after = download(r)
    ref, status = lr.scatter(before, idx, numpy_records(rec))
    same_state(after, ref)
    assert np.array_equal(to_host(rec["status"]).astype(np.uint32), status)
    valid = idx[(idx >= 0) & (idx < N)]
    assert (status == ST_INACTIVE).sum() == idx.size - np.unique(valid).size >= 58 and e.device_views() == views
    # lowest item wins: mean and covariance of a thrice-named filter are those of its first item
    f = int(np.bincount(valid).argmax())
    k = int(np.nonzero(idx == f)[0][0])
    assert (idx == f).sum() >= 3 and np.array_equal(after["mu"][f], to_host(rec["mu"])[k]) and np.array_equal(after["cov"][f], to_host(rec["cov_packed"])[k])
    # a record with initialised == 0 retired its filter; its time is zero whatever the record says
    retired = [int(idx[k]) for k in range(idx.size) if status[k] == 0 and k % 5 == 0]
    assert retired and not after["init"][retired].any() and not after["last_ts"][retired].any() and to_host(rec["last_ts_us"])[::5].all()
    # the owner workspace is released: the same call again decides the same way
    e.scatter_filters_dev(to_dev(idx), **rec)
    same_state(download(r), ref)
    assert np.array_equal(to_host(rec["status"]).astype(np.uint32), status)
    # without the optional fields: flag 1, time 0, latches and noise untouched
    e.scatter_filters_dev(to_dev(idx), mu=rec["mu"], cov_packed=rec["cov_packed"])
    ref2, _ = lr.scatter(ref, idx, {"mu": to_host(rec["mu"]), "cov": to_host(rec["cov_packed"])})
    same_state(download(r), ref2)
    e.close()


@pytest.mark.parametrize("model", MODELS)
def test_scatter_refusals(spe, model):
    r = make(spe, model, N, 0)   # batch-uniform noise
    e = r.e
    rec = records_from(spe, model, 0, 16, seed=14)
    before = download(r)
    with pytest.raises(spe.UkfbError) as err:
        e.scatter_filters_dev(to_dev(np.arange(16, dtype=np.int32)), **rec)
    assert "code 1" in str(err.value) and "ukfb_set_process_noise_per_filter" in str(err.value)
    for missing in ("mu", "cov_packed"):
        args = {k: v for k, v in rec.items() if k not in ("noise", missing)}
        args.setdefault("mu", None); args.setdefault("cov_packed", None)
        with pytest.raises(spe.UkfbError) as err:
            e.scatter_filters_dev(to_dev(np.arange(16, dtype=np.int32)), **args)
        assert "code 1" in str(err.value)
    with pytest.raises(spe.UkfbError) as err:
        e.scatter_filters_dev(None, rec["mu"], rec["cov_packed"], n=-1)
    assert "code 4" in str(err.value)
    e.scatter_filters_dev(None, rec["mu"], rec["cov_packed"], n=0)   # nothing to do
    same_state(download(r), before)   # the storage has not been switched either
    # ... and without the noise the same records are taken
    e.scatter_filters_dev(to_dev(np.arange(16, dtype=np.int32)), **{k: v for k, v in rec.items() if k != "noise"})
    ref, _ = lr.scatter(before, np.arange(16), numpy_records(rec, with_noise=False))
    same_state(download(r), ref)
    e.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pname,prec", PRECS, ids=IDS)
def test_round_trip_is_complete(spe, model, pname, prec):
    """every field of every filter of A gathered and scattered into a fresh engine B: one more cycle gives the same bits on both
    (placement and wave-mates are the same).  B's noise storage holds other matrices before, so a Pose filter's
    acceleration-branch noise must have been rebuilt from the record for the cycle to agree."""
    a = make(spe, model, N, prec, per_filter_noise=True, skip=(500, 503))
    rec = record_buffers(a.e, N)
    a.e.gather_filters_dev(None, **rec)
    b = make(spe, model, N, prec, cycles=False, skip=(0, N))   # nothing initialised
    b.e.set_process_noise(np.repeat(3.0 * b.e.process_noise()[None], N, axis=0))
    b.per_filter_noise = True
    b.e.scatter_filters_dev(None, **rec)
    assert not to_host(rec["status"]).any()
    sa, sb = download(a), download(b)
    same_state(sa, sb, keys=("mu", "cov", "init", "last_ts", "in_a", "in_b", "noise"))
    mu_now = a.e.state(with_cov=False)[0]
    _, _, z, Q = inputs(spe, model, N, 3, mu_now)
    for r in (a, b):   # the latches stay as they are: B's came with the records
        r.e.cycle_timestamps(stamps(N, 2), np.full(N, a.meas, dtype=np.int32), z, Q)
    sa2, sb2 = download(a), download(b)
    same_state(sa2, sb2, keys=("mu", "cov", "init", "last_ts", "status"))
    assert not np.array_equal(sa2["mu"], sa["mu"]) and (sa2["status"][500:503] & ST_UNINITIALISED).all()
    a.e.close(); b.e.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pname,prec", PRECS, ids=IDS)
def test_retire(spe, model, pname, prec):
    r = make(spe, model, N, prec)
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    before = download(r)
    assert before["last_ts"][mask != 0].all()
    r.e.retire_dev(to_dev(mask))
    after = download(r)
    same_state(after, lr.retire(before, mask))
    assert not after["init"][mask != 0].any() and not after["last_ts"][mask != 0].any() and after["init"][mask == 0].all()
    cycle(spe, r, 3, stamped=False)
    assert np.array_equal((r.e.status() & ST_UNINITIALISED) != 0, mask != 0)
    r.e.close()


def kill(r, dead_filters):
    mask = np.zeros(r.n, dtype=np.uint8)
    mask[dead_filters] = 1
    r.e.retire_dev(to_dev(mask))


def compact_case(spe, model, prec, case):
    rng = np.random.default_rng(21)
    big = {"big-1": 1, "big-3": 3, "big-8": 8}
    if case in big:
        group = big[case]
        n = lr.COMPACT_N // group * group
        r = make(spe, model, n, prec, per_filter_noise=group == 3)
        dead_groups = np.nonzero(rng.random(n // group) < 0.4)[0]
        dead = (dead_groups[:, None] * group + np.arange(group)[None]).reshape(-1)
        if group > 1:   # and partly initialised groups: single filters of other groups
            dead = np.union1d(dead, np.nonzero(rng.random(n) < 0.1)[0])
        kill(r, dead)
        return r, group
    r = make(spe, model, N, prec, per_filter_noise=case == "one-hole")
    if case == "all-dead":
        kill(r, np.arange(N))
    elif case == "one-hole":    # one hole at 0 and one live group, the last
        kill(r, np.concatenate([[0], np.arange(2, N - 1)]))
    elif case == "live-prefix":   # nothing moves
        kill(r, np.arange(700, N))
    return r, 1


@pytest.mark.parametrize("case", ["big-1", "big-3", "big-8", "all-live", "all-dead", "one-hole", "live-prefix"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pname,prec", PRECS, ids=IDS)
def test_compact(spe, model, pname, prec, case):
    r, group = compact_case(spe, model, prec, case)
    e, n = r.e, r.n
    before = download(r)
    views = e.device_views()
    new_index = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    old_index = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    live = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    e.compact_dev(group, new_index, old_index, live)
    after = download(r)
    ref, ref_new, ref_old, ref_live = lr.compact(before, group)
    same_state(after, ref)
    assert np.array_equal(to_host(new_index), ref_new) and np.array_equal(to_host(old_index), ref_old) and int(live.item()) == ref_live
    assert e.device_views() == views
    moved = int((ref_new[ref_new >= 0] != np.nonzero(ref_new >= 0)[0]).sum())
    expect = {"all-live": (N, 0), "all-dead": (0, 0), "one-hole": (2, 1), "live-prefix": (700, 0)}
    if case in expect:
        assert (ref_live, moved) == expect[case]
    else:
        assert moved > n // 10 and len(set(before["status"].tolist())) > 1 and before["last_ts"][ref_new >= 0].any()
    # every output is optional, and a compacted engine is a fixed point
    e.compact_dev(group)
    same_state(download(r), ref)
    # the host form, on an engine that has holes again
    kill(r, np.arange(0, n, 2 * group))
    before = download(r)
    got_new, got_old, got_live = e.compact(group)
    ref, ref_new, ref_old, ref_live = lr.compact(before, group)
    same_state(download(r), ref)
    assert np.array_equal(got_new, ref_new) and np.array_equal(got_old, ref_old) and got_live == ref_live
    e.close()


def test_compact_refusals(spe):
    e = spe.BatchPoseUKF(N, precision=0)
    for group in (0, 9, -1, 3, 4, 8):   # 1022 = 2 * 7 * 73
        with pytest.raises(spe.UkfbError) as err:
            e.compact_dev(group)
        assert "code 1" in str(err.value)
    e.compact_dev(2); e.compact_dev(7)
    e.sync()
    e.close()


def test_compact_then_run(spe):
    """fp64 Pose, 4096 filters with per-filter noise, half of them dead: the twin is compacted, its inputs follow through
    old_index, and two fused cycles on the acceleration branch give the same statuses and, to rounding, the same states."""
    n = 4096
    a = make(spe, "pose", n, 0, per_filter_noise=True)
    b = make(spe, "pose", n, 0, per_filter_noise=True)
    dead = np.nonzero(np.random.default_rng(31).random(n) < 0.5)[0]
    kill(a, dead); kill(b, dead)
    new_index = torch.empty((n,), dtype=torch.int32, device="cuda")
    old_index = torch.empty((n,), dtype=torch.int32, device="cuda")
    live = torch.empty((1,), dtype=torch.int64, device="cuda")
    b.e.compact_dev(1, new_index, old_index, live)
    new, old, L = to_host(new_index), to_host(old_index), int(live.item())
    assert L == n - dead.size and (new >= 0).sum() == L and (new[new >= 0] != np.nonzero(new >= 0)[0]).sum() > n // 8
    src = np.where(old >= 0, old, 0)   # the dead slots of B read some filter's inputs: nothing is done with them
    for c in (3, 4):
        acc, _, z, Q = inputs(spe, "pose", n, c, a.e.state(with_cov=False)[0])
        a.e.set_acceleration(acc, ACC_COV); b.e.set_acceleration(acc[src], ACC_COV)
        a.e.cycle(0.01, a.meas, z, Q); b.e.cycle(0.01, b.meas, z[src], Q[src])
        sa, sb = a.e.status(), b.e.status()
        assert np.array_equal(sb[new[new >= 0]], sa[new >= 0]) and not (sa[new >= 0] & ST_UNINITIALISED).any()
        assert (sa[new < 0] & ST_UNINITIALISED).all() and (sb[L:] & ST_UNINITIALISED).all()
    mu_a, cov_a, _ = a.e.state(); mu_b, cov_b, _ = b.e.state()
    keep = new >= 0
    worst = max(float(np.max(np.abs(x[new[keep]] - y[keep]) / (1.0 + np.abs(y[keep])))) for x, y in ((mu_b, mu_a), (cov_b, cov_a)))
    moved_bits = np.array_equal(mu_b[new[keep]], mu_a[keep]) and np.array_equal(cov_b[new[keep]], cov_a[keep])
    print(f"PARITY lifecycle compact-then-run pose f64 n={n} live={L} cycles=2 max scaled |B[new] - A| = {worst:.3e} "
          f"(bound 1e-9; identical bits: {moved_bits})")
    assert worst <= 1e-9
    a.e.close(); b.e.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pname,prec", PRECS, ids=IDS)
def test_birth_without_the_host(spe, model, pname, prec):
    """after a compact the free slots start at *live: index = live + arange(64) is formed on the device and the records of a
    bank's mixture moments (ukfb_bank_combine_dev's outputs as they lie) become filters; the items beyond the capacity are refused"""
    r = make(spe, model, N, prec)
    e = r.e
    kill(r, np.arange(3, N, 25)[:40])   # 40 deaths: L = N - 40, so 24 of 64 births do not fit
    live = torch.zeros((1,), dtype=torch.int64, device="cuda")
    e.compact_dev(1, None, None, live)
    bank = make(spe, model, 256, prec, first=8192)   # 128 tracks of two hypotheses
    mu_t = torch.zeros((128, e.S), dtype=tdt(e), device="cuda")
    cov_t = torch.zeros((128, e.PK), dtype=tdt(e), device="cuda")
    bank.e.bank_combine_dev(2, torch.full((256,), 0.5, dtype=tdt(e), device="cuda"), mu_t, cov_t)
    bank.e.sync()
    index = (live + torch.arange(64, device="cuda")).to(torch.int32)   # no host value in it
    status = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    before = download(r)
    e.scatter_filters_dev(index, mu_t, cov_t, status=status, n=64)
    after = download(r)
    L = N - 40
    assert int(live.item()) == L and before["init"][:L].all() and not before["init"][L:].any()
    ref, st = lr.scatter(before, np.arange(L, L + 64), {"mu": to_host(mu_t)[:64], "cov": to_host(cov_t)[:64]})
    same_state(after, ref)
    assert np.array_equal(to_host(status).astype(np.uint32), st) and (st[:40] == 0).all() and (st[40:] == ST_INACTIVE).all()
    assert after["init"].all() and not after["last_ts"][L:].any() and np.array_equal(after["mu"][L:], to_host(mu_t)[:40])
    cycle(spe, r, 3, stamped=False)   # the newborn run
    assert not (e.status() & ST_UNINITIALISED).any()
    e.close(); bank.e.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pname,prec", PRECS, ids=IDS)
def test_host_forms(spe, model, pname, prec):
    r = make(spe, model, 203, prec, skip=(100, 102))
    e = r.e
    mu, cov, init = e.state()
    ts = e.last_measurement_time()
    idx = np.array([5, 202, -1, 100, 203, 5, 0], dtype=np.int32)
    g_mu, g_cov, g_ts, g_init = e.gather_filters(idx)
    ok = (idx >= 0) & (idx < 203)
    safe = np.where(ok, idx, 0)
    for got, want in ((g_mu, mu), (g_cov, cov), (g_ts, ts), (g_init, init)):
        expect = want[safe].copy()
        expect[~ok] = 0
        assert np.array_equal(got, expect)
    assert all(np.array_equal(x, y) for x, y in zip(e.gather_filters(), (mu, cov, ts, init)))
    # scatter: the records of filters 5 ... 11 onto the list (5 twice: the first wins); values of the storage type survive the doubles
    st = e.scatter_filters(idx, mu[5:12], cov[5:12], ts[5:12] + 1, np.array([1, 1, 1, 1, 1, 1, 0], dtype=np.uint8))
    assert st.tolist() == [0, 0, ST_INACTIVE, 0, ST_INACTIVE, ST_INACTIVE, 0]
    mu2, cov2, init2 = e.state()
    ts2 = e.last_measurement_time()
    for f, k in ((5, 0), (202, 1), (100, 3), (0, 6)):
        assert np.array_equal(mu2[f], mu[5 + k]) and np.array_equal(cov2[f], cov[5 + k])
        assert init2[f] == (k != 6) and ts2[f] == (ts[5 + k] + 1 if k != 6 else 0)
    untouched = np.setdiff1d(np.arange(203), [5, 202, 100, 0])
    assert np.array_equal(mu2[untouched], mu[untouched]) and np.array_equal(ts2[untouched], ts[untouched])
    st = e.scatter_filters(None, mu[:3], cov[:3])   # item k is filter k; flag 1, time 0
    assert not st.any() and e.state(with_cov=False)[1][:3].all() and not e.last_measurement_time()[:3].any()
    e.close()
