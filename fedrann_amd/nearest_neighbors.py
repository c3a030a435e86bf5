"""All-pairs cosine (or, on sparse rows, Jaccard) k-NN on the GPU.

Mirror of the reference's fedrann/nearest_neighbors.py (NNDescent_ava.get_neighbors :22-55), which
wraps pynndescent.NNDescent(...).neighbor_graph.  NN-descent approximates the exact k-NN graph;
this class returns the exact graph (tiled MFMA distance kernel + top-k, see
csrc/fedrann_hip.hip), so the forest / descent hyper-parameters are accepted and ignored.  A sparse matrix
wider than FDR_MAX_DIM columns is searched as it is (csrc/knn_sparse.inc) instead of densified.
metric="jaccard" (pynndescent's sparse_jaccard, which the reference's `metric` argument reaches) searches the sets of
non-zero entries of the rows, always on the sparse route; metric="weighted_jaccard" searches the non-zero entries
with their values (which must not be negative) by weighted Jaccard (Ruzicka) distance, on the sparse route too.
Rows come back ascending by (distance, index); a row's self match is a neighbour like any other,
as in `index.neighbor_graph`.
"""
import logging

import numpy as np
import scipy.sparse as sp

from . import _lib

logger = logging.getLogger("fedrann_amd")


class _NearestNeighbors:
    def get_neighbors(self, ref, que, n_neighbors):
        raise NotImplementedError()


class NNDescent_ava(_NearestNeighbors):
    def get_neighbors(self, data, metric="cosine", *, index_n_neighbors=50, n_trees=300,
                      leaf_size=200, n_iters=None, diversify_prob=1, pruning_degree_multiplier=1.5,
                      low_memory=True, n_jobs=64, seed=683985, verbose=True, context=None):
        if metric not in ("cosine", "jaccard", "weighted_jaccard"):
            raise ValueError("metric must be 'cosine' (the reference's only call, __main__.py:186), 'jaccard' or "
                             "'weighted_jaccard', got %r" % (metric,))
        ctx = context or _lib.default_context()
        if metric in ("jaccard", "weighted_jaccard"):
            # the non-zero entries alone matter (a zero adds nothing to a set, a minimum or a mass): one route at
            # every width, dense input included
            if not sp.issparse(data) and np.ndim(data) != 2:
                raise ValueError("data must be 2-D")
            return self._sparse_neighbors(sp.csr_matrix(data), int(index_n_neighbors), ctx, verbose, metric=metric)
        if sp.issparse(data) and data.ndim == 2 and data.shape[1] > _lib.FDR_MAX_DIM:
            # too wide to densify (F = 2 x sampled k-mers: 1.3 M columns at 100 k reads): the exact search of the
            # sparse rows themselves, same canonical result as the dense route on the densified matrix
            return self._sparse_neighbors(data, int(index_n_neighbors), ctx, verbose)
        if sp.issparse(data):
            data = data.toarray()
        data = np.ascontiguousarray(data, dtype=np.float32)  # pynndescent also casts to float32
        if data.ndim != 2:
            raise ValueError("data must be 2-D")
        n, d = data.shape
        k = int(index_n_neighbors)
        if n < k:
            raise ValueError("n_neighbors (%d) must not exceed the number of rows (%d)" % (k, n))
        if verbose:
            logger.info("exact cosine k-NN on %s: %d rows x %d dims, k = %d (n_trees / leaf_size / "
                        "n_iters are NN-descent parameters and do not apply)",
                        ctx.device_info()["name"], n, d, k)
        nbr_indices, distances = ctx.knn(data, k)
        return nbr_indices, distances

    @staticmethod
    def _sparse_neighbors(data, k, ctx, verbose, metric="cosine"):
        A = data.tocsr(copy=True)  # (the caller's matrix is left as it is)
        A.sum_duplicates()  # canonical: summed duplicates, ascending columns per row
        A.sort_indices()
        if metric in ("jaccard", "weighted_jaccard"):
            A.eliminate_zeros()  # (a stored zero is absent from the set either way)
        n, F = A.shape
        if n < k:
            raise ValueError("n_neighbors (%d) must not exceed the number of rows (%d)" % (k, n))
        if verbose:
            logger.info("exact %s k-NN on %s over the sparse rows: %d rows x %d features, %d stored entries, "
                        "k = %d", metric, ctx.device_info()["name"], n, F, A.nnz, k)
        if metric == "jaccard":
            if not np.all(np.isfinite(A.data)):
                raise ValueError("values must be finite")
            # values=None: every stored entry is present (a cast to float32 could turn a tiny value into 0)
            return ctx.knn_sparse(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, F, k, metric="jaccard")
        return ctx.knn_sparse(A.indptr.astype(np.int64), A.indices.astype(np.int32),
                              np.ascontiguousarray(A.data, dtype=np.float32), F, k, metric=metric)
