"""The weighted Jaccard (Ruzicka) k-NN of sparse rows in plain numpy: what
fdr_knn_sparse_metric(FDR_METRIC_WEIGHTED_JACCARD) must give, bit for bit.

Row r has stored values x_rf >= 0; a stored 0 is an absent entry, values=None means every stored entry is 1.
  mass     A_r    : the float32 chain A <- A + x_rf over the row's stored entries in stored order, from 0
  shared   m(q,t) : the float32 chain m <- m + min(x_qf, x_tf) over the features both rows hold with a value > 0, in
                    ascending feature order, from 0
  union    u      : (float64(A_q) + float64(A_t)) - float64(m)
  distance        : 0 for u == 0, otherwise float32((u - float64(m)) / u)
Neighbours ascend by (distance bits, index), self included.  Every chain below is vectorised ACROSS rows or pairs and
sequential ALONG the chain, one float32 addition per step, so the order of the additions is the definition's.
"""
import numpy as np

from _jaccard_model import top_k


def _rows(indptr, indices, values):
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    values = np.ones(indices.size, np.float32) if values is None else np.asarray(values, np.float32)
    return indptr, indices, values


def masses(indptr, indices, values):
    """float32 [n]: the mass chains."""
    indptr, indices, values = _rows(indptr, indices, values)
    lens = np.diff(indptr)
    A = np.zeros(lens.size, np.float32)
    for j in range(int(lens.max()) if lens.size else 0):
        r = np.flatnonzero(lens > j)
        A[r] = A[r] + values[indptr[r] + j]  # (float32 + float32: one rounding)
    return A


def _postings(indptr, indices, values):
    """The entries with a value > 0, grouped by feature in ascending order: a list of (rows, values) per feature,
    rows ascending."""
    n = indptr.size - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    keep = values > 0
    f, row, v = indices[keep], row[keep], values[keep]
    order = np.lexsort((row, f))
    f, row, v = f[order], row[order], v[order]
    cuts = np.flatnonzero(np.diff(f)) + 1
    return f[np.concatenate([[0], cuts])] if f.size else f, np.split(row, cuts), np.split(v, cuts)


def distances(m, a, b):
    """float32 distances from float32 arrays (broadcast): shared weights m, masses a and b."""
    m = np.asarray(m, np.float32).astype(np.float64)
    u = (np.asarray(a, np.float32).astype(np.float64) + np.asarray(b, np.float32).astype(np.float64)) - m
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (u - m) / u
    return np.where(u == 0, np.float32(0), d.astype(np.float32)).astype(np.float32)


def shared_all(indptr, indices, values):
    """float32 [n, n]: m(q, t) of every pair (small n)."""
    indptr, indices, values = _rows(indptr, indices, values)
    n = indptr.size - 1
    M = np.zeros((n, n), np.float32)
    feats, rows, vals = _postings(indptr, indices, values)
    for i in range(len(feats)):  # ascending features: each pair's chain grows in the definition's order
        r, v = rows[i], vals[i]
        M[np.ix_(r, r)] += np.minimum.outer(v, v)
    return M


def knn_all(indptr, indices, values, n_features, k):
    """Every row against every row (small n)."""
    A = masses(indptr, indices, values)
    D = distances(shared_all(indptr, indices, values), A[:, None], A[None, :])
    n = A.size
    idx = np.empty((n, k), np.int32)
    dist = np.empty((n, k), np.float32)
    for q in range(n):
        idx[q], dist[q] = top_k(np.ascontiguousarray(D[q]), k)
    return idx, dist


def knn_rows(indptr, indices, values, n_features, k, rows):
    """The given query rows against every row, one posting list per feature of the query (large n)."""
    indptr, indices, values = _rows(indptr, indices, values)
    A = masses(indptr, indices, values)
    n = A.size
    feats, prow, pval = _postings(indptr, indices, values)
    at = {int(f): i for i, f in enumerate(feats)}
    idx = np.empty((len(rows), k), np.int32)
    dist = np.empty((len(rows), k), np.float32)
    for i, q in enumerate(rows):
        m = np.zeros(n, np.float32)
        for j in range(indptr[q], indptr[q + 1]):  # (ascending features)
            if values[j] > 0:
                p = at[int(indices[j])]
                m[prow[p]] += np.minimum(values[j], pval[p])
        idx[i], dist[i] = top_k(distances(m, A[q], A), k)
    return idx, dist
