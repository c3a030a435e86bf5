"""The host side of querying the sparse index with rows that are not in it: the argument check of SparseIndex.query
(check_sparse_queries), the exact merge of per-shard lists (distributed.merge_sparse_topk), and the refusal of a target
shard smaller than k.  No GPU."""
import itertools

import numpy as np
import pytest

from fedrann_amd import _lib, distributed

N, F = 50, 1000


def _q(rows, values=True):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.array([i for r in rows for i in r], np.int32)
    return indptr, indices, (np.linspace(0.5, 2.0, indices.size).astype(np.float32) if values else None)


def test_check_sparse_queries_accepts():
    for metric in _lib.SPARSE_METRICS:
        assert _lib.check_sparse_queries(N, F, metric, np.zeros(1, np.int64), np.zeros(0, np.int32), None, 5) == (0, 5)
        assert _lib.check_sparse_queries(N, F, metric, *_q([[], [3, 9, 999], [], [0]]), 50) == (4, 50)
        assert _lib.check_sparse_queries(N, F, metric, *_q([[1, 2], []], values=False), np.int64(1)) == (2, 1)
    # more query rows than index rows, and a k above the number of queries
    assert _lib.check_sparse_queries(3, F, "cosine", *_q([[1]] * 7), 3) == (7, 3)
    assert _lib.check_sparse_queries(N, F, "jaccard", *_q([[1]]), 20) == (1, 20)


def test_check_sparse_queries_refuses():
    indptr, indices, values = _q([[1, 2, 7], [4]])
    ok = lambda metric="cosine", n=N, f=F, ip=indptr, ix=indices, v=values, k=5: \
        _lib.check_sparse_queries(n, f, metric, ip, ix, v, k)
    assert ok() == (2, 5)
    with pytest.raises(ValueError, match="k"):
        ok(k=N + 1)
    with pytest.raises(ValueError, match="k"):
        ok(n=500, k=_lib.FDR_MAX_K + 1)
    with pytest.raises(ValueError, match="k"):
        ok(k=0)
    with pytest.raises(ValueError, match="k"):
        ok(k=2.0)
    with pytest.raises(ValueError, match="outside"):
        ok(f=7)  # an id >= n_features
    with pytest.raises(ValueError, match="ascending"):
        ok(ix=np.array([2, 1, 7, 4], np.int32))
    with pytest.raises(ValueError, match="ascending"):
        ok(ix=np.array([1, 1, 7, 4], np.int32))
    nan = values.copy()
    nan[1] = np.nan
    neg = values.copy()
    neg[3] = -0.5
    for metric in _lib.SPARSE_METRICS:
        with pytest.raises(ValueError, match="finite"):
            ok(metric, v=nan)
    with pytest.raises(ValueError, match="negative"):
        ok("weighted_jaccard", v=neg)
    assert ok("cosine", v=neg) == (2, 5) and ok("jaccard", v=neg) == (2, 5)  # (refused under weighted_jaccard only)
    with pytest.raises(ValueError, match="metric"):
        ok("euclid")
    with pytest.raises(TypeError):
        ok(ip=indptr.astype(np.int32))
    with pytest.raises(TypeError):
        ok(ix=indices.astype(np.int64))
    with pytest.raises(TypeError):
        ok(v=values.astype(np.float64))
    with pytest.raises(TypeError):
        ok(ix=list(indices))
    with pytest.raises(ValueError, match="row pointer"):
        ok(ip=np.array([0, 3, 5], np.int64))
    with pytest.raises(ValueError, match="row pointer"):
        ok(ip=np.array([1, 3, 4], np.int64))


def _brute(idx, dist, k):
    out_i = np.empty((idx.shape[0], k), np.int32)
    out_d = np.empty((idx.shape[0], k), np.float32)
    for q in range(idx.shape[0]):
        order = np.lexsort((idx[q], dist[q].view(np.uint32)))[:k]
        out_i[q], out_d[q] = idx[q][order], dist[q][order]
    return out_i, out_d


def _parts(seed, nq=40, widths=(20, 20, 7)):
    """Per-shard lists over disjoint target ranges: many tied distances, rows at exactly 1.0, each list ascending by
    (distance bits, index) as a search leaves it."""
    rng = np.random.default_rng(seed)
    parts, base = [], 0
    for w in widths:
        idx = np.stack([base + np.sort(rng.choice(1000, w, replace=False)) for _ in range(nq)]).astype(np.int32)
        dist = rng.choice(np.array([0.0, 0.25, 0.25, 0.5, 0.75, 1.0, 1.0, 1.0], np.float32), size=(nq, w))
        dist[rng.random((nq, w)) < 0.2] = np.float32(1.0) - np.float32(2.0 ** -24)  # just below 1
        i, d = _brute(idx, dist.astype(np.float32), w)
        parts.append((i, d))
        base += 1000
    return parts


@pytest.mark.parametrize("k", [1, 7, 40])
def test_merge_sparse_topk_is_the_brute_force_order(k):
    parts = _parts(seed=k)
    want = _brute(np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1), k)
    assert k < 40 or np.any(want[1] == 1.0)  # (the rows at exactly 1 are merged in index order too)
    for perm in itertools.permutations(range(len(parts))):
        got = distributed.merge_sparse_topk([parts[i] for i in perm], k)
        assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == got[1].shape == (40, k)
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    with pytest.raises(ValueError):
        distributed.merge_sparse_topk([], k)
    with pytest.raises(ValueError):
        distributed.merge_sparse_topk(parts, 48)  # more than the lists hold


def test_target_shard_smaller_than_k_is_refused_without_a_context():
    indptr, indices, values = _q([[i % 9, 10 + i % 7] for i in range(100)])
    # shard_rows(100, 3): 64 rows, 36 rows, none
    for rank, k in ((0, 65), (1, 37), (2, 1)):
        with pytest.raises(ValueError, match="target rows"):
            distributed.sparse_knn_target_shard(None, indptr, indices, values, F, k, rank, 3)
    with pytest.raises(ValueError):
        distributed.sparse_knn_target_shard(None, indptr, indices, values, F, 5, 3, 3)  # no such rank
