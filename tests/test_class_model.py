"""The model of the duplicate-row class layer (tests/_class_model.py) is right: on small sparse inputs with duplicates
the oracle's k-NN over the UNIQUE rows, expanded by the model, is the oracle's k-NN over ALL rows bit for bit, and the
model's classification of the lists finds every kind of stratum there.  No GPU: this is what settles, when
tests/test_gpu_class_expand.py fails, that the kernel is wrong and not the model."""
import numpy as np
import pytest

import _class_lists as L
import _class_model as M

KS = (1, 3, 20, 33)
INPUTS = [(600, 32, 1), (450, 16, 2), (333, 32, 3)]

_cases = {}  # (n, d, seed) -> the rows, their classes and the unique rows' lists per k: made once, read-only


def _case(oracle, n, d, seed):
    if (n, d, seed) not in _cases:
        Eh, _, zero = oracle.normalize(M.hot_rows(n, d, seed))
        cls_of_row, members, reps = M.classes_of(Eh)
        lists = {k: oracle.knn_normalized(Eh[reps], zero[reps], Eh[reps], zero[reps], k) for k in KS}
        _cases[(n, d, seed)] = (Eh, zero, cls_of_row, members, reps, lists)
    return _cases[(n, d, seed)]


@pytest.mark.parametrize("n,d,seed", INPUTS)
def test_expanded_unique_lists_are_the_full_search(oracle, n, d, seed):
    Eh, zero, cls_of_row, members, reps, lists = _case(oracle, n, d, seed)
    size = np.array([len(m) for m in members])
    assert len(members) < n and size.max() >= 20 and np.sum(size == 1) >= 40, (len(members), size.max())
    assert np.array_equal(reps, np.sort(reps)) and np.array_equal(cls_of_row[reps], np.arange(len(reps)))
    assert sorted(np.concatenate(members).tolist()) == list(range(n))
    for k in KS:
        iu, du = lists[k]
        # (the kernel's precondition, and the reason classes are numbered by representative)
        key = (du.view(np.uint32).astype(np.uint64) << np.uint64(32)) | iu.astype(np.uint64)
        assert np.all(key[:, 1:] > key[:, :-1])
        for q0, nq, t_base in ((0, n, 0), (n // 3, n // 2, 1 << 20)):
            gi, gb = M.expand(members, cls_of_row, iu, du, q0, nq, k, t_base)
            wi, wd = oracle.knn_normalized(Eh[q0:q0 + nq], zero[q0:q0 + nq], Eh, zero, k, t_base=t_base)
            bad = np.flatnonzero(np.any(gi != wi, axis=1) | np.any(gb != wd.view(np.uint32), axis=1))
            assert bad.size == 0, "k = %d: %d rows differ, the first %d" % (k, bad.size, q0 + int(bad[0]))


def test_every_kind_of_stratum_is_met(oracle):
    """fast, concat and a tie stratum hold queries of these inputs at every k that has one, and over all k at least two
    tie strata do; no query lands in a stratum that reachable(k) rules out"""
    total = dict.fromkeys(M.STRATA, 0)
    for k in KS:
        c = dict.fromkeys(M.STRATA, 0)
        for n, d, seed in INPUTS:
            _, _, cls_of_row, members, _, lists = _case(oracle, n, d, seed)
            one = M.counts(M.path_of(members, lists[k][0], lists[k][1], k, cls_of_row))
            print("n = %d d = %d k = %d: %s" % (n, d, k, one))
            assert sum(one.values()) == n and all(one[s] == 0 for s in M.STRATA if s not in M.reachable(k)), (k, one)
            c = {s: c[s] + one[s] for s in M.STRATA}
        assert c["fast"] > 0 and c["concat"] > 0, (k, c)
        assert k == 1 or any(c[s] > 0 for s in M.TIE_STRATA), (k, c)
        total = {s: total[s] + c[s] for s in M.STRATA}
    assert sum(total[s] > 0 for s in M.TIE_STRATA) >= 2, total


def test_classes_compare_bits():
    T = np.zeros((6, 4), dtype=np.float32)
    T[1, 2] = -0.0
    T[2] = T[4] = [1, 2, 3, 4]
    T[5, 2] = -0.0
    cls_of_row, members, reps = M.classes_of(T)
    assert cls_of_row.tolist() == [0, 1, 2, 0, 2, 1] and reps.tolist() == [0, 1, 2]
    assert [m.tolist() for m in members] == [[0, 3], [1, 5], [2, 4]]


def test_reachable_and_path_by_hand():
    assert M.reachable(1) == ("fast", "concat")
    assert M.reachable(2) == M.reachable(5) == ("fast", "concat", "sort32")       # n <= 4, n <= 25
    assert M.reachable(6) == ("fast", "concat", "sort32", "sort64")               # n <= 36
    assert M.reachable(11) == ("fast", "concat", "sort32", "sort64", "sort128")   # n <= 121
    assert M.reachable(12) == M.reachable(31) == M.STRATA                          # 144 > 128; n = 32 is a sort32
    assert M.reachable(32) == ("fast", "concat", "sort64", "sort128", "select")   # n >= 33
    assert M.reachable(63) == ("fast", "concat", "sort64", "sort128", "select")   # n = 64: one class of two
    assert M.reachable(64) == ("fast", "concat", "sort128", "select")
    one, two = np.uint32(0x3F800000), np.uint32(0x40000000)
    assert M.path_one([1, 1, 1], [one, one, one], 3) == "fast"
    assert M.path_one([1, 2, 1], [0, one, two], 3) == "concat"
    assert M.path_one([1, 2, 1], [0, one, one], 3) == "sort32"
    assert M.path_one([3, 1, 1], [0, one, one], 3) == "concat"      # the tie lies behind the first k elements
    assert M.path_one([2, 1, 1], [0, one, one], 3) == "sort32"      # base_1 = 2 < 3
    assert M.path_one([2], [0], 1) == "concat" and M.path_one([1], [0], 1) == "fast"
    assert M.path_one([40, 40] + [1] * 38, [0] * 40, 40) == "sort128"  # n = 118
    assert M.path_one([40, 40, 40] + [1] * 37, [0] * 40, 40) == "select"
    members = [np.array([0, 5, 9]), np.array([1]), np.array([2, 3])]
    idx, bits = M.expand_one(members, [0, 2, 1], [7, 7, 9], 3, t_base=100)
    assert idx.tolist() == [100, 102, 103] and bits.tolist() == [7, 7, 7]


@pytest.mark.parametrize("k", L.KS)
def test_synthetic_lists_meet_the_floor(k):
    """The made-up targets and lists tests/test_gpu_class_expand.py hands the kernel, with its seeds: classes of the
    intended sizes, the signed-zero pair apart, and the floor per reachable stratum and for mixed waves (L.condition)."""
    T = L.target_rows(k, 128, seed=k)
    cls_of_row, members, _ = M.classes_of(T)
    size = sorted(len(m) for m in members)
    assert size[-3:] == [200, 200, 700] and sum(size) == L.N and {k, k + 1} <= set(size)
    ids, bits = L.lists(members, k, seed=1000 + k)
    paths_u = M.path_of(members, ids, bits, k)
    cu, cq, mixed = L.condition(k, paths_u, paths_u[cls_of_row])
    print("k = %d: %d classes; lists per stratum %s; queries per stratum %s; mixed %s" % (k, len(members), cu, cq, mixed))
