"""The Jaccard k-NN of sparse rows in plain numpy / scipy: what fdr_knn_sparse_metric(FDR_METRIC_JACCARD) must give.

A row's set is its stored entries whose value is not 0 (every stored entry when values is None).  For query q and
target t with a = |S_q|, b = |S_t|, c = |S_q & S_t| and u = a + b - c, the distance is 0 for u = 0 and otherwise
np.float32(np.float64(u - c) / np.float64(u)); neighbours ascend by (distance bits, index), self included.
"""
import numpy as np
import scipy.sparse as sp


def binary_csr(indptr, indices, values, n_features):
    """B: the binary CSR (int64 ones) of the present entries."""
    n = indptr.size - 1
    data = np.ones(indices.size, np.int64) if values is None else (np.asarray(values) != 0).astype(np.int64)
    B = sp.csr_matrix((data, np.asarray(indices, np.int64), np.asarray(indptr, np.int64)), shape=(n, n_features))
    B.eliminate_zeros()
    return B


def distances(c, a, b):
    """float32 distances from int64 arrays (broadcast): shared counts c, set sizes a and b."""
    c = np.asarray(c, np.int64)
    u = np.asarray(a, np.int64) + np.asarray(b, np.int64) - c
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (u - c).astype(np.float64) / u.astype(np.float64)
    return np.where(u == 0, np.float32(0), d.astype(np.float32)).astype(np.float32)


def top_k(dist, k):
    """(idx int32 [k], dist float32 [k]) of one query's float32 distances to every row, by (dist bits, index)."""
    bits = dist.view(np.uint32)
    order = np.lexsort((np.arange(dist.size), bits))[:k]
    return order.astype(np.int32), dist[order]


def knn_all(indptr, indices, values, n_features, k):
    """Every row against every row through B @ B.T (small n)."""
    B = binary_csr(indptr, indices, values, n_features)
    sizes = np.asarray(B.getnnz(1), np.int64)
    C = np.asarray((B @ B.T).todense(), np.int64)
    D = distances(C, sizes[:, None], sizes[None, :])
    n = B.shape[0]
    idx = np.empty((n, k), np.int32)
    dist = np.empty((n, k), np.float32)
    for q in range(n):
        idx[q], dist[q] = top_k(np.ascontiguousarray(D[q]), k)
    return idx, dist


def knn_rows(indptr, indices, values, n_features, k, rows):
    """The given query rows against every row, one CSC column slice per query (large n)."""
    B = binary_csr(indptr, indices, values, n_features)
    sizes = np.asarray(B.getnnz(1), np.int64)
    Bc = B.tocsc()
    n = B.shape[0]
    idx = np.empty((len(rows), k), np.int32)
    dist = np.empty((len(rows), k), np.float32)
    for i, q in enumerate(rows):
        cols = B.indices[B.indptr[q]:B.indptr[q + 1]]
        c = np.asarray(Bc[:, cols].sum(axis=1), np.int64).ravel() if cols.size else np.zeros(n, np.int64)
        idx[i], dist[i] = top_k(distances(c, sizes[q], sizes), k)
    return idx, dist
