"""Query rows against a separate set of target rows, in numpy / scipy and the oracle: what fdr_sparse_index_query must
give, bit for bit, from models that know nothing of the kernel.

  cosine            both sets densified over the union of their distinct ids in ascending order (every chain keeps its
                    order and terms), oracle.normalize on each, oracle.knn_normalized(queries, targets)
  Jaccard,          the stacked CSR [targets; queries] through the pieces of _jaccard_model / _weighted_jaccard_model;
  weighted Jaccard  a query row's distance vector is cut to the first n columns (the targets) before top_k
A CSR is (indptr, indices, values); values may be None (every stored entry 1) on either side.
"""
import numpy as np
import scipy.sparse as sp

import _jaccard_model as jm
import _weighted_jaccard_model as wm


def _ones(csr):
    indptr, indices, values = csr
    return indptr, indices, (np.ones(indices.size, np.float32) if values is None else values)


def _dense(csr, pool):
    indptr, indices, values = csr
    D = np.zeros((indptr.size - 1, pool.size), np.float32)
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    D[rows, np.searchsorted(pool, indices)] = values
    return D


def stack(targets, queries):
    """(indptr, indices, values) of [targets; queries]; values None only where both sides have none."""
    if targets[2] is not None or queries[2] is not None:
        targets, queries = _ones(targets), _ones(queries)
    indptr = np.concatenate([targets[0], targets[0][-1] + queries[0][1:]]).astype(np.int64)
    indices = np.concatenate([targets[1], queries[1]]).astype(np.int32)
    values = None if targets[2] is None else np.concatenate([targets[2], queries[2]]).astype(np.float32)
    return indptr, indices, values


def cosine(oracle, targets, queries, k):
    targets, queries = _ones(targets), _ones(queries)
    pool = np.unique(np.concatenate([targets[1], queries[1]]))
    if pool.size == 0:
        pool = np.zeros(1, np.int32)
    Th, _, tzero = oracle.normalize(_dense(targets, pool))
    Qh, _, qzero = oracle.normalize(_dense(queries, pool))
    return oracle.knn_normalized(Qh, qzero, Th, tzero, k)


def jaccard_distances(targets, queries, n_features):
    """float32 [nq, n]: every query against every target."""
    n, nq = targets[0].size - 1, queries[0].size - 1
    B = jm.binary_csr(*stack(targets, queries), n_features)
    sizes = np.asarray(B.getnnz(1), np.int64)
    Bc = B.tocsc()
    D = np.empty((nq, n), np.float32)
    for i in range(nq):
        cols = B.indices[B.indptr[n + i]:B.indptr[n + i + 1]]
        c = np.asarray(Bc[:, cols].sum(axis=1), np.int64).ravel() if cols.size else np.zeros(n + nq, np.int64)
        D[i] = jm.distances(c, sizes[n + i], sizes)[:n]
    return D


def weighted_jaccard_distances(targets, queries):
    """float32 [nq, n]: every query against every target."""
    n, nq = targets[0].size - 1, queries[0].size - 1
    indptr, indices, values = wm._rows(*stack(targets, queries))
    A = wm.masses(indptr, indices, values)
    feats, prow, pval = wm._postings(indptr, indices, values)
    at = {int(f): i for i, f in enumerate(feats)}
    D = np.empty((nq, n), np.float32)
    for i in range(nq):
        m = np.zeros(n + nq, np.float32)
        for j in range(indptr[n + i], indptr[n + i + 1]):  # (ascending features)
            if values[j] > 0:
                p = at[int(indices[j])]
                m[prow[p]] += np.minimum(values[j], pval[p])
        D[i] = wm.distances(m, A[n + i], A)[:n]
    return D


def top_k_rows(D, k):
    idx = np.empty((D.shape[0], k), np.int32)
    dist = np.empty((D.shape[0], k), np.float32)
    for i in range(D.shape[0]):
        idx[i], dist[i] = jm.top_k(np.ascontiguousarray(D[i]), k)
    return idx, dist


def check_cosine_rows(oracle, row_norms, targets, queries, n_features, k, rows, got):
    """The sampled query rows, each against every target restricted to the query's own features (the only terms its
    chains have): what _check_queries of test_gpu_sparse_knn does for own rows, with the query's rinv taken from its
    own row.  row_norms: that module's _row_norms."""
    n = targets[0].size - 1
    rinv_t, zero_t = row_norms(oracle, targets[0], targets[2])
    rinv_q, zero_q = row_norms(oracle, queries[0], queries[2])
    A = sp.csr_matrix((targets[2], targets[1], targets[0]), shape=(n, n_features)).tocsc()
    for q in rows:
        a, b = queries[0][q], queries[0][q + 1]
        cols = queries[1][a:b]
        if cols.size == 0:
            Th = np.zeros((n, 1), np.float32)
            Qh = np.zeros((1, 1), np.float32)
        else:
            Th = (A[:, cols].toarray().astype(np.float32) * rinv_t[:, None]).astype(np.float32)
            Qh = (queries[2][a:b] * rinv_q[q]).astype(np.float32)[None, :]
        wi, wd = oracle.knn_normalized(Qh, zero_q[q:q + 1], Th, zero_t, k)
        assert np.array_equal(got[0][q], wi[0]), "query %d: %s vs %s" % (q, got[0][q], wi[0])
        assert np.array_equal(got[1][q].view(np.uint32), wd[0].view(np.uint32)), "query %d distances" % q
