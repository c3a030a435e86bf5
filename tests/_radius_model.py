"""Radius search in numpy: what fdr_sparse_index_radius_search / _radius_query must give, bit for bit, from the models
of the k-NN search (_sparse_query_model), which know nothing of the kernel.

A result is a ragged CSR (indptr int64 [nq + 1], idx int32 [total], dist float32 [total]): row i holds every target
with distance <= r, ordered by (distance bits, index) ascending -- the k-NN order.  Distances are never negative, so
the order of the bit patterns is the order of the values.

  Jaccard, weighted Jaccard   rows_within(D, r) on the full float32 [nq, n] matrix of jaccard_distances /
                              weighted_jaccard_distances
  cosine                      cosine_ranked ranks ALL n targets per query (the oracle at k = n), cut_ranked keeps each
                              row's prefix with distance <= r
"""
import numpy as np

import _sparse_query_model as qmodel


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    if rows:
        np.cumsum([r[0].size for r in rows], out=indptr[1:])
    idx = np.concatenate([r[0] for r in rows]).astype(np.int32) if rows else np.zeros(0, np.int32)
    dist = np.concatenate([r[1] for r in rows]).astype(np.float32) if rows else np.zeros(0, np.float32)
    return indptr, idx, dist


def rows_within(D, r):
    """D float32 [nq, n] -> the ragged result at radius r."""
    D = np.ascontiguousarray(D, dtype=np.float32)
    r = np.float32(r)
    rows = []
    for i in range(D.shape[0]):
        sel = np.flatnonzero(D[i] <= r)
        bits = D[i, sel].view(np.uint32)
        order = np.lexsort((sel, bits))  # (last key first: distance bits, then index)
        rows.append((sel[order], D[i, sel[order]]))
    return _csr(rows)


def cut_ranked(idx, dist, r):
    """(idx, dist) [nq, n], each row ALL targets in (distance bits, index) order -> the ragged result at radius r."""
    r = np.float32(r)
    rows = []
    for i in range(idx.shape[0]):
        keep = dist[i] <= r
        c = int(keep.sum())
        assert keep[:c].all()  # a prefix: the row is ascending
        rows.append((idx[i, :c], dist[i, :c]))
    return _csr(rows)


def cosine_ranked(oracle, targets, queries):
    return qmodel.cosine(oracle, targets, queries, k=targets[0].size - 1)


def cosine_rows(oracle, targets, queries, r):
    return cut_ranked(*cosine_ranked(oracle, targets, queries), r)


def distances(metric, targets, queries, n_features):
    """The full matrix under "jaccard" or "weighted_jaccard"."""
    if metric == "jaccard":
        return qmodel.jaccard_distances(targets, queries, n_features)
    assert metric == "weighted_jaccard"
    return qmodel.weighted_jaccard_distances(targets, queries)


def model(metric, oracle, targets, queries, n_features):
    """r -> the ragged result; the expensive part (the matrix, the oracle's ranking) is computed once."""
    if metric == "cosine":
        ranked = cosine_ranked(oracle, targets, queries)
        return lambda r: cut_ranked(*ranked, r)
    D = distances(metric, targets, queries, n_features)
    return lambda r: rows_within(D, r)


def same(got, want):
    """Equal indptr, equal indices, equal distance bit patterns."""
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert np.array_equal(got[0], want[0]), "indptr differs (totals %d vs %d)" % (got[0][-1], want[0][-1])
    assert np.array_equal(got[1], want[1]), "indices differ"
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "distance bits differ"
