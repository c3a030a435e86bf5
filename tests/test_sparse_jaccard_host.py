"""The Jaccard model of tests/_jaccard_model.py against Python set arithmetic and scikit-learn, and the argument
handling of the Python layer and the command line for the Jaccard search.  Needs no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import _jaccard_model as model
from fedrann_amd import _lib

F = 40


def _hand_rows():
    """62 small rows as (ids, values): empty rows, explicit zeros, exact duplicates, equal sets under different
    values, nested subsets, disjoint rows."""
    rng = np.random.default_rng(4)
    rows = []
    for i in range(40):
        m = int(rng.integers(1, 9))
        ids = np.sort(rng.choice(F - 8, m, replace=False))
        vals = rng.integers(1, 5, size=m).astype(np.float32) * rng.choice([-1.0, 1.0], size=m).astype(np.float32)
        vals[rng.random(m) < 0.2] = 0.0
        rows.append((ids, vals))
    rows += [(np.zeros(0, np.int64), np.zeros(0, np.float32))] * 3  # empty
    rows += [(np.array([1, 2, 3]), np.zeros(3, np.float32))] * 2  # stored zeros only: empty sets
    rows += [rows[0], rows[0], (rows[1][0], np.where(rows[1][1] != 0, 7.0, -0.0).astype(np.float32))]  # duplicates
    base = np.arange(F - 8, F)
    rows += [(base[:j], np.ones(j, np.float32)) for j in range(1, 9)]  # nested subsets
    rows += [(base[6:], np.ones(2, np.float32)), (base[::2], np.ones(4, np.float32)),
             (base[1::2], np.ones(4, np.float32)), (np.array([0]), np.ones(1, np.float32)),
             (np.array([0, F - 1]), np.array([0.0, 2.0], np.float32)), (np.array([5]), np.array([-0.0], np.float32))]
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r[0]) for r in rows])
    indices = np.concatenate([r[0] for r in rows]).astype(np.int32)
    values = np.concatenate([r[1] for r in rows]).astype(np.float32)
    return rows, indptr, indices, values


@pytest.fixture(scope="module")
def hand():
    return _hand_rows()


def _brute(rows, k):
    sets = [set(int(f) for f, v in zip(ids, vals) if v != 0) for ids, vals in rows]
    n = len(sets)
    idx = np.empty((n, k), np.int32)
    dist = np.empty((n, k), np.float32)
    for q in range(n):
        keys = []
        for t in range(n):
            u = len(sets[q] | sets[t])
            c = len(sets[q] & sets[t])
            d = np.float32(0.0) if u == 0 else np.float32(np.float64(u - c) / np.float64(u))
            keys.append((int(np.array(d, np.float32).view(np.uint32)), t, d))
        keys.sort()
        idx[q] = [t for _, t, _ in keys[:k]]
        dist[q] = [d for _, _, d in keys[:k]]
    return idx, dist


@pytest.mark.parametrize("k", [1, 7, 62])
def test_model_matches_set_arithmetic(hand, k):
    rows, indptr, indices, values = hand
    assert len(rows) == 62
    wi, wd = _brute(rows, k)
    gi, gd = model.knn_all(indptr, indices, values, F, k)
    assert np.array_equal(gi, wi)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
    ri, rd = model.knn_rows(indptr, indices, values, F, k, list(range(len(rows))))
    assert np.array_equal(ri, wi)
    assert np.array_equal(rd.view(np.uint32), wd.view(np.uint32))


def test_model_without_values_counts_every_stored_entry(hand):
    rows, indptr, indices, _ = hand
    ones = [(ids, np.ones(len(ids), np.float32)) for ids, _ in rows]
    wi, wd = _brute(ones, 10)
    gi, gd = model.knn_all(indptr, indices, None, F, 10)
    assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def test_model_distances_match_sklearn(hand):
    from sklearn.metrics import pairwise_distances
    _, indptr, indices, values = hand
    B = model.binary_csr(indptr, indices, values, F)
    sizes = np.asarray(B.getnnz(1), np.int64)
    C = np.asarray((B @ B.T).todense(), np.int64)
    D = model.distances(C, sizes[:, None], sizes[None, :])
    want = pairwise_distances(B.toarray().astype(bool), metric="jaccard").astype(np.float32)
    assert np.array_equal(D.view(np.uint32), want.view(np.uint32))
    assert D[40, 41] == 0.0 and D[40, 0] == 1.0  # two empty rows; an empty row and a non-empty one


def test_equal_ratios_from_different_counts_tie_on_the_bits():
    assert model.distances(1, 1, 2).view(np.uint32) == model.distances(2, 2, 4).view(np.uint32)
    idx, dist = model.top_k(model.distances(np.array([2, 1, 0, 1]), 2, np.array([4, 1, 3, 1])), 4)
    assert idx.tolist() == [0, 1, 3, 2] and dist.tolist() == [0.5, 0.5, 0.5, 1.0]


# ---- the Python layer and the command line, without a context ----------------------------------------------------------
def _ctx_without_gpu():
    return _lib.Context.__new__(_lib.Context)  # (knn_sparse checks its arguments before it touches the library)


@pytest.mark.parametrize("metric", ["euclidean", "Jaccard", "", None, 1])
def test_unknown_metric_is_a_value_error(metric):
    indptr = np.array([0, 1, 2], np.int64)
    indices = np.array([0, 1], np.int32)
    with pytest.raises(ValueError, match="cosine.*jaccard"):
        _ctx_without_gpu().knn_sparse(indptr, indices, None, 4, 1, metric=metric)


def test_jaccard_arguments_are_checked_like_cosine():
    indptr = np.array([0, 2, 3], np.int64)
    with pytest.raises(ValueError, match="ascending"):
        _ctx_without_gpu().knn_sparse(indptr, np.array([3, 1, 0], np.int32), None, 4, 1, metric="jaccard")
    with pytest.raises(ValueError, match="finite"):
        _ctx_without_gpu().knn_sparse(indptr, np.array([0, 1, 0], np.int32), np.array([1, np.inf, 1], np.float32), 4,
                                      1, metric="jaccard")


def test_metric_codes_match_the_header():
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "fedrann_hip.h")).read()
    assert int(re.search(r"#define FDR_METRIC_COSINE (\d+)", hdr).group(1)) == _lib.SPARSE_METRICS["cosine"]
    assert int(re.search(r"#define FDR_METRIC_JACCARD (\d+)", hdr).group(1)) == _lib.SPARSE_METRICS["jaccard"]


def test_nndescent_lists_the_supported_metrics():
    from fedrann_amd.nearest_neighbors import NNDescent_ava
    with pytest.raises(ValueError) as e:
        NNDescent_ava().get_neighbors(sp.csr_matrix((4, 8), dtype=np.float32), metric="euclidean", index_n_neighbors=2)
    assert "cosine" in str(e.value) and "jaccard" in str(e.value)


def test_cli_metric_needs_no_projection(tmp_path):
    from fedrann_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["-o", str(tmp_path / "out"), "--feature-matrix", "x.npz", "--kmer-counts", "c.npy",
              "--no-projection-metric", "jaccard"])
    assert e.value.code not in (0, None)
    assert "--no-projection-metric" in str(e.value.code) and "--no-projection " in str(e.value.code) + " "
    assert not (tmp_path / "out").exists()  # (refused before any work)


def test_cli_default_metric_is_cosine():
    from fedrann_amd.__main__ import parse_command_line_arguments
    assert parse_command_line_arguments(["-o", "x"]).no_projection_metric == "cosine"
    assert parse_command_line_arguments(["-o", "x", "--no-projection", "--no-projection-metric",
                                         "jaccard"]).no_projection_metric == "jaccard"
    with pytest.raises(SystemExit):
        parse_command_line_arguments(["-o", "x", "--no-projection", "--no-projection-metric", "hamming"])
