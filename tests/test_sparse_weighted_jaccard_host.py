"""The weighted Jaccard model of tests/_weighted_jaccard_model.py on hand-computed cases, against a scalar restatement
and against the Jaccard model, the monotonicity property the definition rests on, and the argument handling of the
Python layer and the command line for the weighted Jaccard search.  Needs no GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _jaccard_model as jaccard
import _weighted_jaccard_model as model
from _weighted_rows import csr, weighted_rows
from fedrann_amd import _lib

f32 = np.float32


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _row(ids, vals):
    return np.array(ids, np.int64), np.array(vals, np.float32)


# ---- the model on hand-computed cases ------------------------------------------------------------------------------------
def test_two_rows_with_known_min_and_max_sums():
    # minima 1 + 1 = 2, maxima 2 + 3 + 4 + 2 = 11, masses 7 and 6: dist = 9 / 11
    rows = csr([_row([1, 3, 5], [2, 1, 4]), _row([1, 3, 7], [1, 3, 2])])
    assert model.masses(*rows).tolist() == [7.0, 6.0]
    assert model.shared_all(*rows).tolist() == [[7.0, 2.0], [2.0, 6.0]]
    idx, dist = model.knn_all(*rows, 8, 2)
    assert idx.tolist() == [[0, 1], [1, 0]]
    assert np.array_equal(_bits(dist), _bits([[0.0, f32(9.0 / 11.0)]] * 2))
    ri, rd = model.knn_rows(*rows, 8, 2, [1, 0])
    assert np.array_equal(ri, idx[[1, 0]]) and np.array_equal(_bits(rd), _bits(dist[[1, 0]]))


def test_a_stored_zero_is_absent():
    rows = csr([_row([1, 3], [2.0, 0.0]), _row([3], [5.0]), _row([1], [2.0]), _row([1, 3], [2.0, -0.0])])
    idx, dist = model.knn_all(*rows, 4, 4)
    assert idx[0].tolist() == [0, 2, 3, 1] and dist[0].tolist() == [0.0, 0.0, 0.0, 1.0]  # (feature 3 is not shared)
    assert idx[1].tolist() == [1, 0, 2, 3] and dist[1].tolist() == [0.0, 1.0, 1.0, 1.0]


def test_zero_mass_rows_and_duplicates():
    rows = csr([_row([], []), _row([2, 4], [0.0, -0.0]), _row([2, 4], [1.5, 0.25]), _row([2, 4], [1.5, 0.25]),
                _row([4], [0.25])])
    assert model.masses(*rows).tolist() == [0.0, 0.0, 1.75, 1.75, 0.25]
    idx, dist = model.knn_all(*rows, 8, 5)
    assert idx[0].tolist() == [0, 1, 2, 3, 4] and dist[0].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0]  # two zero-mass rows: 0
    assert idx[1].tolist() == [0, 1, 2, 3, 4] and dist[1].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0]
    assert idx[2].tolist() == [2, 3, 4, 0, 1] and idx[3].tolist() == [2, 3, 4, 0, 1]  # duplicates: 0, in index order
    assert np.array_equal(_bits(dist[2]), _bits([0.0, 0.0, f32(1.5 / 1.75), 1.0, 1.0]))
    assert dist[4].tolist()[:1] == [0.0] and idx[4].tolist() == [4, 2, 3, 0, 1]


def test_the_chains_are_float32_and_ordered():
    # 2^24 + 1 + 1 in float32 stays 2^24 (each step rounds), 1 + 1 + 2^24 is 2^24 + 2: the order is the definition's
    big = float(1 << 24)
    rows = csr([_row([0, 1, 2], [big, 1, 1]), _row([0, 1, 2], [1, 1, big])])
    assert model.masses(*rows).tolist() == [big, big + 2]
    M = model.shared_all(*rows)
    assert M[0, 1] == 3.0 and M[0, 0] == big and M[1, 1] == big + 2  # minima 1, 1, 1
    d = model.distances(M[0, 1], big, big + 2)
    u = (np.float64(big) + np.float64(big + 2)) - 3.0
    assert _bits(d) == _bits(f32((u - 3.0) / u))


def _scalar_knn(rows, k):
    """The definition, one pair and one float32 addition at a time."""
    mass = []
    for ids, vals in rows:
        a = f32(0)
        for v in vals:
            a = f32(a + f32(v))
        mass.append(a)
    n = len(rows)
    idx = np.empty((n, k), np.int32)
    dist = np.empty((n, k), np.float32)
    for q in range(n):
        qd = {int(f): f32(v) for f, v in zip(*rows[q]) if v > 0}
        keys = []
        for t in range(n):
            m = f32(0)
            for f, v in zip(*rows[t]):  # (ascending features)
                if v > 0 and int(f) in qd:
                    m = f32(m + min(qd[int(f)], f32(v)))
            u = (np.float64(mass[q]) + np.float64(mass[t])) - np.float64(m)
            d = f32(0) if u == 0 else f32((u - np.float64(m)) / u)
            keys.append((int(_bits(d)), t, d))
        keys.sort()
        idx[q] = [t for _, t, _ in keys[:k]]
        dist[q] = [d for _, _, d in keys[:k]]
    return idx, dist


@pytest.fixture(scope="module")
def rows500():
    return weighted_rows(500, seed=77, F=1 << 20, n_ids=160)


def test_model_matches_the_scalar_definition():
    indptr, indices, values = weighted_rows(150, seed=5, F=4096, n_ids=64, per=(1, 9))
    rows = [(indices[indptr[i]:indptr[i + 1]], values[indptr[i]:indptr[i + 1]]) for i in range(150)]
    wi, wd = _scalar_knn(rows, 40)
    gi, gd = model.knn_all(indptr, indices, values, 4096, 40)
    assert np.array_equal(gi, wi) and np.array_equal(_bits(gd), _bits(wd))
    ri, rd = model.knn_rows(indptr, indices, values, 4096, 40, list(range(150)))
    assert np.array_equal(ri, wi) and np.array_equal(_bits(rd), _bits(wd))
    assert np.unique(wd).size > 20  # (weights at work: more distances than the few a handful of set sizes give)


def test_all_ones_values_give_the_jaccard_bits(rows500):
    indptr, indices, values = rows500
    F = 1 << 20
    ji, jd = jaccard.knn_all(indptr, indices, None, F, 64)
    for v in (None, np.ones(indices.size, np.float32)):
        gi, gd = model.knn_all(indptr, indices, v, F, 64)
        assert np.array_equal(gi, ji) and np.array_equal(_bits(gd), _bits(jd))
    some = (values != 0).astype(np.float32)  # (stored zeros among the ones: absent under both measures)
    ji, jd = jaccard.knn_all(indptr, indices, some, F, 64)
    gi, gd = model.knn_all(indptr, indices, some, F, 64)
    assert np.array_equal(gi, ji) and np.array_equal(_bits(gd), _bits(jd))
    wi, _ = model.knn_all(indptr, indices, values, F, 64)
    assert np.any(wi != ji)  # (the weights change the answer)


def test_shared_weight_never_exceeds_either_mass_on_the_bits(rows500):
    indptr, indices, values = rows500
    rng = np.random.default_rng(3)
    # values without a grid: float32 numbers whose sums round at every step
    rough = np.where(values > 0, rng.random(values.size).astype(np.float32) * values, values).astype(np.float32)
    for v in (values, rough):
        A = model.masses(indptr, indices, v)
        M = model.shared_all(indptr, indices, v)
        assert np.all(M <= np.minimum(A[:, None], A[None, :]))
        assert np.array_equal(_bits(np.diag(M)), _bits(A + f32(0)))  # a row against itself: its own mass
        D = model.distances(M, A[:, None], A[None, :])
        assert np.all((D >= 0) & (D <= 1)) and np.all(np.diag(D) == 0)
        assert np.array_equal(_bits(D), _bits(D.T))  # (min and the fp64 sum commute)


# ---- the Python layer and the command line, without a context ----------------------------------------------------------
def _ctx_without_gpu():
    return _lib.Context.__new__(_lib.Context)  # (knn_sparse checks its arguments before it touches the library)


def test_metric_code_matches_the_header():
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "fedrann_hip.h")).read()
    code = int(re.search(r"#define FDR_METRIC_WEIGHTED_JACCARD (\d+)", hdr).group(1))
    assert code == _lib.METRIC_WEIGHTED_JACCARD == _lib.SPARSE_METRICS["weighted_jaccard"] == 2
    assert _lib.sparse_metric_code("weighted_jaccard") == code
    with pytest.raises(ValueError, match="cosine.*jaccard.*weighted_jaccard"):
        _lib.sparse_metric_code("ruzicka")


@pytest.mark.parametrize("bad, what", [([1.0, -0.5, 1.0], "negative"), ([1.0, np.nan, 1.0], "finite"),
                                       ([3e38, 3e38, 1.0], "finite"), ([1.0, np.inf, 1.0], "finite")])
def test_bad_values_are_refused_before_the_library(bad, what):
    indptr = np.array([0, 2, 3], np.int64)
    indices = np.array([0, 1, 0], np.int32)
    values = np.array(bad, np.float32)
    with pytest.raises(ValueError, match=what):
        _ctx_without_gpu().knn_sparse(indptr, indices, values, 4, 1, metric="weighted_jaccard")
    with pytest.raises(ValueError, match=what):
        _ctx_without_gpu().sparse_index(indptr, indices, values, 4, metric="weighted_jaccard")
    with pytest.raises(ValueError, match=what):
        _lib.check_sparse_rows(indptr, indices, values, 4, 1, metric="weighted_jaccard")
    with pytest.raises(ValueError, match=what):
        _lib.check_sparse_csr(indptr, indices, values, 4, metric="weighted_jaccard")


def test_the_other_metrics_and_positional_calls_keep_their_checks():
    indptr = np.array([0, 2, 3], np.int64)
    indices = np.array([0, 1, 0], np.int32)
    neg = np.array([1.0, -0.5, 1.0], np.float32)
    huge = np.array([3e38, 3e38, 1.0], np.float32)
    for v in (neg, huge):
        assert _lib.check_sparse_rows(indptr, indices, v, 4, 1) == (2, 1, 4)
        assert _lib.check_sparse_csr(indptr, indices, v, 4) == (2, 4)
        assert _lib.check_sparse_rows(indptr, indices, v, 4, 1, metric="jaccard") == (2, 1, 4)
    # accepted under the weighted metric: -0, a mass just below the float32 maximum, no values at all, empty rows
    ok = np.array([3e38, 4e37, -0.0], np.float32)
    assert _lib.check_sparse_rows(indptr, indices, ok, 4, 1, metric="weighted_jaccard") == (2, 1, 4)
    assert _lib.check_sparse_rows(indptr, indices, None, 4, 1, metric="weighted_jaccard") == (2, 1, 4)
    empty = np.array([0, 0, 3, 3], np.int64)
    assert _lib.check_sparse_csr(empty, np.array([0, 1, 2], np.int32), ok, 4, metric="weighted_jaccard") == (3, 4)
    with pytest.raises(ValueError, match="finite"):  # (the overflowing pair in one row, between two empty rows)
        _lib.check_sparse_csr(empty, np.array([0, 1, 2], np.int32), huge, 4, metric="weighted_jaccard")
    with pytest.raises(ValueError, match="ascending"):
        _ctx_without_gpu().knn_sparse(indptr, np.array([3, 1, 0], np.int32), None, 4, 1, metric="weighted_jaccard")


def test_cli_accepts_the_metric_and_still_needs_no_projection(tmp_path):
    from fedrann_amd.__main__ import main, parse_command_line_arguments
    args = parse_command_line_arguments(["-o", "x", "--no-projection", "--no-projection-metric", "weighted_jaccard"])
    assert args.no_projection_metric == "weighted_jaccard" and args.no_projection
    with pytest.raises(SystemExit) as e:
        main(["-o", str(tmp_path / "out"), "--feature-matrix", "x.npz", "--kmer-counts", "c.npy",
              "--no-projection-metric", "weighted_jaccard"])
    assert e.value.code not in (0, None) and "--no-projection-metric weighted_jaccard" in str(e.value.code)
    assert not (tmp_path / "out").exists()


def test_cli_stage_two_clamps_negative_idf_weights(tmp_path):
    from fedrann_amd.__main__ import load_inputs
    from fedrann_amd.feature_extraction import save_feature_matrix_npz
    from fedrann_amd.precompute import idf_weights
    from fedrann_amd.synth import synth
    s = synth(300, seed=9, doubling=True)
    counts = s["counts"].copy()
    counts[3] = s["n_features"] + 5  # ln(F / count) < 0 for this k-mer and its reverse complement
    fm, cnt = str(tmp_path / "feature_matrix.npz"), str(tmp_path / "counts.npy")
    save_feature_matrix_npz(fm, s["indptr"], s["indices"], s["n_features"])
    np.save(cnt, counts)
    kw = dict(output_dir=str(tmp_path), embedding_dimension=8, save_feature_matrix=False, feature_matrix=fm,
              kmer_counts=cnt, no_projection=True)
    idf = idf_weights(counts, s["n_features"])
    assert int(np.sum(idf < 0)) == 2
    w = load_inputs(metric="weighted_jaccard", **kw)[3]
    assert w.dtype == np.float32 and np.array_equal(_bits(w), _bits(np.maximum(idf, f32(0))))
    assert w.min() == 0 and int(np.sum(w == 0)) == 2
    assert np.array_equal(_bits(load_inputs(metric="cosine", **kw)[3]), _bits(idf))  # (cosine keeps the sign)


def test_nndescent_accepts_the_name():
    from fedrann_amd.nearest_neighbors import NNDescent_ava
    A = sp.csr_matrix(np.array([[1, 0, 2], [0, -1, 0], [3, 0, 0], [0, 0, 1]], np.float32))
    # the name passes the metric check and reaches the value checks of the sparse route (no GPU touched before them)
    for data in (A, A.toarray()):
        with pytest.raises(ValueError, match="negative"):
            NNDescent_ava().get_neighbors(data, metric="weighted_jaccard", index_n_neighbors=2,
                                          context=_ctx_without_gpu(), verbose=False)
    with pytest.raises(ValueError, match="cosine.*jaccard"):
        NNDescent_ava().get_neighbors(A, metric="euclidean", index_n_neighbors=2, context=_ctx_without_gpu())
