"""The radius model itself (tests/_radius_model.py), the wrapper's argument checks and the cutting of an over-cap block
into pieces: numpy only, no GPU."""
import numpy as np
import pytest

import _radius_model as rmodel
import _sparse_query_model as qmodel
from _weighted_rows import csr as rows_csr
from fedrann_amd import _lib


def _small_sets(seed, n, nq, n_ids=40):
    """Random sets over few ids (many shared features, ties in the distances), some of them empty."""
    rng = np.random.default_rng(seed)

    def rows(m):
        out = []
        for i in range(m):
            ids = np.sort(rng.choice(n_ids, int(rng.integers(0, 9)), replace=False)).astype(np.int64)
            out.append((ids, (0.25 * rng.integers(1, 5, ids.size)).astype(np.float32)))
        return rows_csr(out)
    return rows(n), rows(nq)


@pytest.mark.parametrize("metric", ["jaccard", "weighted_jaccard"])
def test_model_rows_are_prefixes_of_the_knn_model(metric):
    """Wherever a radius row has at most k entries it is the prefix, with distance <= r, of the k-NN model's row; a
    longer one starts with all k of them."""
    targets, queries = _small_sets(3, 300, 60)
    D = rmodel.distances(metric, targets, queries, 64)
    assert D.dtype == np.float32 and D.shape == (60, 300)
    short = longer = 0
    for r in (0.0, 0.5, 0.9, 0.97):
        indptr, idx, dist = rmodel.rows_within(D, r)
        assert indptr[0] == 0 and indptr[-1] == idx.size == dist.size == int((D <= np.float32(r)).sum())
        for k in (1, 20, 128):
            ki, kd = qmodel.top_k_rows(D, k)
            for i in range(60):
                a, b = indptr[i], indptr[i + 1]
                m = min(k, b - a)
                keep = kd[i] <= np.float32(r)
                assert int(keep.sum()) == m and keep[:m].all()
                assert np.array_equal(idx[a:a + m], ki[i, :m])
                assert np.array_equal(dist[a:a + m].view(np.uint32), kd[i, :m].view(np.uint32))
                short += b - a <= k
                longer += b - a > k
        keys = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
        for i in range(60):
            assert np.all(np.diff(keys[indptr[i]:indptr[i + 1]].astype(np.int64)) > 0)
        assert not np.any(dist == 1.0)
    assert short > 100 and longer > 100


def test_cut_ranked_is_rows_within_on_a_ranking():
    targets, queries = _small_sets(4, 200, 30)
    D = rmodel.distances("jaccard", targets, queries, 64)
    ranked = qmodel.top_k_rows(D, 200)
    for r in (0.0, 0.6, 0.95):
        rmodel.same(rmodel.cut_ranked(*ranked, r), rmodel.rows_within(D, r))


def test_radius_argument_checks():
    assert _lib.check_sparse_radius(0.0) == (np.float32(0.0), 1 << 26)
    assert _lib.check_sparse_radius(np.float32(0.97), 5) == (np.float32(0.97), 5)
    for bad in (float("nan"), -0.1, 1.0, float("inf"), 1.5, None, "0.5", True):
        with pytest.raises(ValueError, match="radius"):
            _lib.check_sparse_radius(bad)
    for bad in (0, -1, 1 << 31, 2.5, None, True):
        with pytest.raises(ValueError, match="max_hits"):
            _lib.check_sparse_radius(0.5, bad)


def test_radius_pieces_cover_the_rows_and_fit_the_cap():
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 50, 400)
    for cap in (49, 50, 200, 10 ** 6):
        pieces = _lib.radius_pieces(counts, cap)
        assert pieces[0][0] == 0 and pieces[-1][1] == 400
        assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
        assert all(a < b and counts[a:b].sum() <= cap for a, b in pieces)
        # greedy: no piece could have taken the next row as well
        assert all(counts[a:b + 1].sum() > cap for a, b in pieces[:-1])
    assert _lib.radius_pieces(counts, int(counts.max()) - 1) is None
    assert _lib.radius_pieces(np.zeros(0, np.int64), 5) == [(0, 0)]
    assert _lib.radius_pieces(np.array([5, 0, 0, 5, 1]), 5) == [(0, 3), (3, 4), (4, 5)]
