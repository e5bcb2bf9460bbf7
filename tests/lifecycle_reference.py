"""NumPy reference of the filter lifecycle (include/ukf_batch.h, "filter lifecycle"): gather, scatter (lowest item wins), retire
and compact on a dict of per-filter arrays.  Nothing here computes with a scalar, every operation moves bits, so the device's
results must equal these bit for bit.

The engine as a dict ("state"): mu [N, S], cov [N, PK], init uint8 [N], last_ts int64 [N], status uint32 [N], in_a / in_b
[N, 3] (the engine-owned latches), noise [N, D, D] (per filter) or [D, D] (batch-uniform) and, Pose engines with per-filter noise,
racc [N, D, D].  Any key may be missing; what is missing is not moved.  No function changes its arguments."""
import numpy as np

ST_INACTIVE = 1 << 8
# capacity of the GPU compact test (tests/test_gpu_lifecycle.py): odd, 40 count blocks of 1024 groups with a ragged last one at
# group = 1 and still more than three at group = 8; tests/test_lifecycle_host.py holds the host geometry to that
COMPACT_N = 40003
FIELDS = ("mu", "cov", "last_ts", "init", "in_a", "in_b", "noise")


def copy_state(state):
    return {k: np.array(v, copy=True) for k, v in state.items()}


def valid_items(index, capacity):
    index = np.asarray(index, dtype=np.int64)
    return (index >= 0) & (index < capacity)


def gather(state, index, fields=FIELDS, in_a_read=None, in_b_read=None):
    """records of the items of `index` (None: item k is filter k): a dict of `fields` and "status".  in_a_read / in_b_read: the
    bound buffers, where the next prediction reads them instead of the latches."""
    n_filters = state["init"].shape[0]
    index = np.arange(n_filters) if index is None else np.asarray(index, dtype=np.int64)
    ok = valid_items(index, n_filters)
    safe = np.where(ok, index, 0)
    out = {}
    for f in fields:
        src = state[f]
        if f == "in_a" and in_a_read is not None:
            src = in_a_read
        if f == "in_b" and in_b_read is not None:
            src = in_b_read
        if f == "noise" and src.ndim == 2:
            src = np.broadcast_to(src, (n_filters,) + src.shape)
        rows = np.array(src[safe], copy=True)
        rows[~ok] = 0
        out[f] = rows
    out["status"] = np.where(ok, 0, ST_INACTIVE).astype(np.uint32)
    return out


def racc_of(noise, acc_cov):
    """the acceleration-branch form of noise matrices [.., D, D]: block (6, 6, 3, 3) = T(2) * T(acc_cov), in the matrices' type"""
    out = np.array(noise, copy=True)
    t = out.dtype.type
    out[..., 6:9, 6:9] = t(2) * np.asarray(acc_cov, dtype=out.dtype)
    return out


def scatter(state, index, rec, acc_cov=None):
    """-> (state after, per-item status).  rec: mu and cov, optionally init (None / missing: 1), last_ts (missing: 0), in_a, in_b,
    noise.  Among the valid items that name one filter the lowest item index wins and writes the whole record."""
    new = copy_state(state)
    n_filters = state["init"].shape[0]
    n = rec["mu"].shape[0]
    index = np.arange(n) if index is None else np.asarray(index, dtype=np.int64)
    status = np.full(n, ST_INACTIVE, dtype=np.uint32)
    taken = set()
    for k in range(n):
        f = int(index[k])
        if f < 0 or f >= n_filters or f in taken:
            continue
        taken.add(f)
        status[k] = 0
        flag = 1 if rec.get("init") is None else int(rec["init"][k] != 0)
        new["mu"][f] = rec["mu"][k]
        new["cov"][f] = rec["cov"][k]
        new["init"][f] = flag
        new["last_ts"][f] = int(rec["last_ts"][k]) if (flag and rec.get("last_ts") is not None) else 0
        for key in ("in_a", "in_b"):
            if rec.get(key) is not None:
                new[key][f] = rec[key][k]
        if rec.get("noise") is not None:
            assert new["noise"].ndim == 3, "noise records need per-filter storage"
            new["noise"][f] = rec["noise"][k]
            if "racc" in new:
                new["racc"][f] = racc_of(rec["noise"][k], acc_cov)
    return new, status


def retire(state, mask):
    new = copy_state(state)
    dead = np.asarray(mask) != 0
    new["init"][dead] = 0
    new["last_ts"][dead] = 0
    return new


def compact(state, group=1):
    """-> (state after, new_index int32 [N], old_index int32 [N], live).  Group g (filters g * group ... g * group + group - 1) is
    live if any of its filters is initialised; L live groups; the dead groups below L (holes) receive, in ascending order, the live
    groups at or above L (movers) in ascending order."""
    new = copy_state(state)
    init = state["init"]
    n = init.shape[0]
    assert 1 <= group <= 8 and n % group == 0
    G = n // group
    live = init.reshape(G, group).any(axis=1)
    L = int(live.sum())
    holes = [g for g in range(L) if not live[g]]
    movers = [g for g in range(L, G) if live[g]]
    assert len(holes) == len(movers)
    new_index = np.full(n, -1, dtype=np.int32)
    old_index = np.full(n, -1, dtype=np.int32)
    for g in range(L):
        if live[g]:
            sl = np.arange(g * group, (g + 1) * group)
            new_index[sl] = sl
            old_index[sl] = sl
    per_filter = [k for k in ("mu", "cov", "init", "last_ts", "status", "in_a", "in_b", "racc") if k in state]
    if "noise" in state and state["noise"].ndim == 3:
        per_filter.append("noise")
    for h, m in zip(holes, movers):
        src = np.arange(m * group, (m + 1) * group)
        dst = np.arange(h * group, (h + 1) * group)
        for key in per_filter:
            new[key][dst] = state[key][src]
        new["init"][src] = 0
        new["last_ts"][src] = 0
        new_index[src] = dst
        old_index[dst] = src
    return new, new_index, old_index, L * group
