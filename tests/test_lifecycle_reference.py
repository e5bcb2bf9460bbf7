"""tests/lifecycle_reference.py pinned by hand-written cases: every expected array below is written out, none is computed."""
import numpy as np

import lifecycle_reference as lr

ST_INACTIVE = 1 << 8


def tiny_state(flags, S=2, PK=3, D=2, per_filter_noise=True, racc=False):
    """filter i carries the value i + 1 in every scalar (mu: i + 1, cov: 10 (i + 1), ...): a moved record is recognisable"""
    flags = np.asarray(flags, dtype=np.uint8)
    n = flags.size
    tag = np.arange(1, n + 1, dtype=np.float64)
    s = {"mu": np.repeat(tag[:, None], S, 1), "cov": np.repeat(10 * tag[:, None], PK, 1), "init": flags.copy(),
         "last_ts": (1000 * tag).astype(np.int64) * flags, "status": (tag.astype(np.uint32) << 16),
         "in_a": np.repeat(0.5 * tag[:, None], 3, 1), "in_b": np.repeat(-0.5 * tag[:, None], 3, 1)}
    s["noise"] = np.repeat(100 * tag[:, None], D * D, 1).reshape(n, D, D) if per_filter_noise else np.full((D, D), 7.0)
    if racc:
        s["racc"] = -s["noise"]
    return s


def tags(state):
    return state["mu"][:, 0].astype(int).tolist()


def test_compact_seven_groups():
    s = tiny_state([0, 1, 0, 1, 1, 0, 1], racc=True)
    new, new_index, old_index, live = lr.compact(s, 1)
    assert live == 4
    # holes (0, 2) receive movers (4, 6)
    assert new_index.tolist() == [-1, 1, -1, 3, 0, -1, 2]
    assert old_index.tolist() == [4, 1, 6, 3, -1, -1, -1]
    assert new["init"].tolist() == [1, 1, 1, 1, 0, 0, 0]
    assert new["last_ts"].tolist() == [5000, 2000, 7000, 4000, 0, 0, 0]
    # the movers keep their other bits; the dead group 5 keeps everything
    assert tags(new) == [5, 2, 7, 4, 5, 6, 7]
    assert new["cov"][:, 0].tolist() == [50, 20, 70, 40, 50, 60, 70]
    assert (new["status"] >> 16).tolist() == [5, 2, 7, 4, 5, 6, 7]
    assert new["in_a"][:, 2].tolist() == [2.5, 1.0, 3.5, 2.0, 2.5, 3.0, 3.5]
    assert new["in_b"][:, 0].tolist() == [-2.5, -1.0, -3.5, -2.0, -2.5, -3.0, -3.5]
    assert new["noise"][:, 1, 1].tolist() == [500, 200, 700, 400, 500, 600, 700]
    assert new["racc"][:, 0, 1].tolist() == [-500, -200, -700, -400, -500, -600, -700]
    # the argument is untouched
    assert s["init"].tolist() == [0, 1, 0, 1, 1, 0, 1] and tags(s) == [1, 2, 3, 4, 5, 6, 7]


def test_compact_uniform_noise_is_not_moved():
    s = tiny_state([0, 1], per_filter_noise=False)
    new, new_index, old_index, live = lr.compact(s, 1)
    assert live == 1 and new_index.tolist() == [-1, 0] and old_index.tolist() == [1, -1]
    assert np.array_equal(new["noise"], np.full((2, 2), 7.0)) and tags(new) == [2, 2]


def test_compact_all_live_and_all_dead():
    s = tiny_state([1, 1, 1, 1, 1])
    new, new_index, old_index, live = lr.compact(s, 1)
    assert live == 5 and new_index.tolist() == [0, 1, 2, 3, 4] and old_index.tolist() == [0, 1, 2, 3, 4]
    assert all(np.array_equal(new[k], s[k]) for k in s)
    s = tiny_state([0, 0, 0, 0, 0])
    new, new_index, old_index, live = lr.compact(s, 1)
    assert live == 0 and new_index.tolist() == [-1] * 5 and old_index.tolist() == [-1] * 5
    assert all(np.array_equal(new[k], s[k]) for k in s)


def test_compact_groups_of_three_partly_initialised():
    # groups: (0 0 0) dead, (0 1 0) live, (0 0 0) dead, (1 0 1) live, (0 0 1) live  ->  L = 3, hole 0 <- mover 3, hole 2 <- mover 4
    flags = [0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1]
    s = tiny_state(flags)
    new, new_index, old_index, live = lr.compact(s, 3)
    assert live == 9
    assert new_index.tolist() == [-1, -1, -1, 3, 4, 5, -1, -1, -1, 0, 1, 2, 6, 7, 8]
    assert old_index.tolist() == [9, 10, 11, 3, 4, 5, 12, 13, 14, -1, -1, -1, -1, -1, -1]
    assert new["init"].tolist() == [1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert new["last_ts"].tolist() == [10000, 0, 12000, 0, 5000, 0, 0, 0, 15000, 0, 0, 0, 0, 0, 0]
    assert tags(new) == [10, 11, 12, 4, 5, 6, 13, 14, 15, 10, 11, 12, 13, 14, 15]


def test_retire():
    s = tiny_state([1, 1, 0, 1])
    new = lr.retire(s, [1, 0, 1, 0])
    assert new["init"].tolist() == [0, 1, 0, 1] and new["last_ts"].tolist() == [0, 2000, 0, 4000]
    assert all(np.array_equal(new[k], s[k]) for k in s if k not in ("init", "last_ts"))


def test_gather_with_invalid_items_and_a_bound_buffer():
    s = tiny_state([1, 0, 1], per_filter_noise=False)
    bound = np.array([[9.0, 9, 9], [8, 8, 8], [7, 7, 7]])
    rec = lr.gather(s, [2, -1, 0, 3, 2], in_a_read=bound)
    assert rec["status"].tolist() == [0, ST_INACTIVE, 0, ST_INACTIVE, 0]
    assert rec["mu"][:, 0].tolist() == [3, 0, 1, 0, 3] and rec["cov"][:, 2].tolist() == [30, 0, 10, 0, 30]
    assert rec["init"].tolist() == [1, 0, 1, 0, 1] and rec["last_ts"].tolist() == [3000, 0, 1000, 0, 3000]
    assert rec["in_a"][:, 1].tolist() == [7, 0, 9, 0, 7] and rec["in_b"][:, 1].tolist() == [-1.5, 0, -0.5, 0, -1.5]
    assert rec["noise"][:, 0, 0].tolist() == [7, 0, 7, 0, 7]   # the uniform matrix for a valid item
    assert np.array_equal(lr.gather(s, None)["mu"], s["mu"])


def test_scatter_triple_duplicate_and_two_invalid_items():
    s = tiny_state([1, 1, 1, 1], racc=True)
    s["noise"] = np.zeros((4, 12, 12)); s["racc"] = np.zeros((4, 12, 12))
    index = [2, 4, 2, 0, -3, 2, 3]
    n = len(index)
    rec = {"mu": np.repeat(np.arange(100.0, 100 + n)[:, None], 2, 1), "cov": np.repeat(np.arange(200.0, 200 + n)[:, None], 3, 1),
           "init": np.array([1, 1, 1, 0, 1, 1, 7], dtype=np.uint8), "last_ts": np.arange(1, n + 1, dtype=np.int64) * 11,
           "in_a": np.full((n, 3), 1.0) * np.arange(n)[:, None], "noise": np.ones((n, 12, 12)) * np.arange(1, n + 1)[:, None, None]}
    acc_cov = np.arange(1.0, 10.0).reshape(3, 3)
    new, status = lr.scatter(s, index, rec, acc_cov=acc_cov)
    # item 0 wins filter 2 over items 2 and 5; items 1 and 4 are invalid; item 3 retires filter 0; item 6 (flag 7 -> 1) takes filter 3
    assert status.tolist() == [0, ST_INACTIVE, ST_INACTIVE, 0, ST_INACTIVE, ST_INACTIVE, 0]
    assert new["mu"][:, 0].tolist() == [103, 2, 100, 106] and new["cov"][:, 0].tolist() == [203, 20, 200, 206]
    assert new["init"].tolist() == [0, 1, 1, 1] and new["last_ts"].tolist() == [0, 2000, 11, 77]
    assert new["in_a"][:, 0].tolist() == [3, 1.0, 0, 6] and np.array_equal(new["in_b"], s["in_b"])
    assert new["noise"][:, 0, 0].tolist() == [4, 0, 1, 7]
    assert new["racc"][:, 0, 0].tolist() == [4, 0, 1, 7] and new["racc"][:, 6, 5].tolist() == [4, 0, 1, 7]
    assert new["racc"][:, 6, 6].tolist() == [2, 0, 2, 2] and new["racc"][:, 8, 7].tolist() == [16, 0, 16, 16]
    assert new["racc"][:, 9, 9].tolist() == [4, 0, 1, 7]
    assert np.array_equal(new["status"], s["status"])   # the engine's own status words are not written
    # without the optional fields: flag 1, time 0, latches and noise untouched
    new, status = lr.scatter(s, [1, 1], {"mu": rec["mu"][:2], "cov": rec["cov"][:2]})
    assert status.tolist() == [0, ST_INACTIVE] and new["mu"][:, 0].tolist() == [1, 100, 3, 4]
    assert new["init"].tolist() == [1, 1, 1, 1] and new["last_ts"].tolist() == [1000, 0, 3000, 4000]
    assert np.array_equal(new["in_a"], s["in_a"]) and np.array_equal(new["noise"], s["noise"])
