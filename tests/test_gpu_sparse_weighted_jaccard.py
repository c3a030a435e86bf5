"""Exact weighted Jaccard k-NN on sparse feature rows (fdr_knn_sparse_metric, FDR_METRIC_WEIGHTED_JACCARD): indices and
distance bits against the numpy model of tests/_weighted_jaccard_model.py -- every row of a hard set, n == k, tie
plateaus, long queries, the range-split path, all-ones values against metric="jaccard", the index and the ranks of a
world, argument errors, NNDescent_ava(metric="weighted_jaccard") and the --no-projection-metric command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import _weighted_jaccard_model as model
from _weighted_rows import csr, weighted_rows
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WJ = "weighted_jaccard"


def _same(a, b):
    ai, ad = a
    bi, bd = b
    assert ai.shape == bi.shape
    bad = np.flatnonzero(np.any((ai != bi) | (ad.view(np.uint32) != bd.view(np.uint32)), axis=1))
    assert bad.size == 0, "rows differ: %s (first: got %s %s, want %s %s)" % (
        bad[:10], ai[bad[0]], ad[bad[0]], bi[bad[0]], bd[bad[0]])


def _same_rows(got, rows, want):
    _same((got[0][rows], got[1][rows]), want)


# ---- 1. every row against the model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hard():
    rows = weighted_rows(4000, seed=1701)
    want = model.knn_all(*rows, 1 << 25, 128)  # (a prefix of the (dist, index) order is the smaller k's answer)
    return rows, want


@pytest.mark.parametrize("k", [1, 20, 64, 128])
def test_every_row_matches_the_model(ctx, hard, k):
    (indptr, indices, values), (wi, wd) = hard
    got = ctx.knn_sparse(indptr, indices, values, 1 << 25, k, metric=WJ)
    assert ctx.last_knn_trace()["kind"] == "sparse"
    _same(got, (wi[:, :k], wd[:, :k]))


def test_trace_counts_the_zero_mass_rows(ctx, hard):
    (indptr, indices, values), _ = hard
    ctx.knn_sparse(indptr, indices, values, 1 << 25, 20, metric=WJ)
    A = model.masses(indptr, indices, values)
    t = ctx.last_knn_trace()
    assert t["zero_queries"] == int(np.sum(A == 0)) > int(np.sum(np.diff(indptr) == 0)) > 0, t  # (rows of +-0 too)
    assert t["kind"] == "sparse" and t["queries"] == t["targets"] == 4000 and t["k"] == 20, t


# ---- 2. n == k --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 128])
def test_n_equals_k(ctx, n):
    indptr, indices, values = weighted_rows(n, seed=n, F=1 << 24, n_ids=128, per=(1, 4))
    _same(ctx.knn_sparse(indptr, indices, values, 1 << 24, n, metric=WJ),
          model.knn_all(indptr, indices, values, 1 << 24, n))


def test_denormal_values_are_kept(ctx):
    """Values, masses and minima below the smallest normal float32 (1.18e-38): a flush to zero anywhere in S1w or S3w
    would turn these rows into zero-mass rows."""
    indptr, indices, values = weighted_rows(300, seed=41, F=1 << 20, n_ids=96, per=(1, 6))
    tiny = (values / np.float32(0.37) * np.float32(3e-41)).astype(np.float32)  # multiples of a denormal step
    A = model.masses(indptr, indices, tiny)
    assert 0 < A.max() < np.finfo(np.float32).tiny and np.sum(A > 0) > 200
    _same(ctx.knn_sparse(indptr, indices, tiny, 1 << 20, 20, metric=WJ), model.knn_all(indptr, indices, tiny, 1 << 20, 20))


# ---- 3. tie plateaus --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plateaus():
    """3000 rows, each a subset of 8 ids (the empty subset included) with one weight per id, as IDF weights are:
    weights 1, 1, 2, 2, 3, 3, 4, 4 (times 0.25), so that different subsets have equal masses and equal shared
    weights, and every distance is a ratio of small integers."""
    rng = np.random.default_rng(8)
    ids = np.sort(rng.choice(1 << 20, 8, replace=False)).astype(np.int64)
    w = (np.array([1, 1, 2, 2, 3, 3, 4, 4]) * 0.25).astype(np.float32)
    masks = rng.integers(0, 256, size=3000)
    rows = [((m >> np.arange(8)) & 1) == 1 for m in masks]
    rows = [(ids[r], w[r]) for r in rows]
    rows_csr = csr(rows)
    return rows_csr, model.knn_all(*rows_csr, 1 << 20, 128)


@pytest.mark.parametrize("k", [20, 128])
def test_tie_plateaus_keep_the_index_order(ctx, plateaus, k):
    (indptr, indices, values), (wi, wd) = plateaus
    # masses and shared weights are integers up to 20 (times 0.25, exact in float32): the distances are fractions
    # 1 - m / u with m <= u <= 20, at most the 129 terms of the Farey sequence of order 20 for 3000 * 128 entries,
    # so the neighbours lie on plateaus and the index order decides
    assert np.unique(wd).size <= 129 and np.any(wd == np.float32(0.5))
    assert np.unique(model.masses(indptr, indices, values)).size <= 21
    got = ctx.knn_sparse(indptr, indices, values, 1 << 20, k, metric=WJ)
    _same(got, (wi[:, :k], wd[:, :k]))


# ---- 4. long queries --------------------------------------------------------------------------------------------------
def test_long_queries(ctx):
    """1-300 entries from 2000 ids: the query walk takes several 64-entry rounds.  Every fourth row is short (its
    table comes close to SP_LIMIT = 512 targets, on either side), every fourth is long over 6000 ids of its own kind
    (several rounds into one table of at most 375 targets); the rest pass SP_LIMIT and take the range split."""
    rng = np.random.default_rng(15)
    n, F = 1500, 8000
    rows = []
    for i in range(n):
        if i % 4 == 1:
            ids = 2000 + np.sort(rng.choice(6000, int(rng.integers(70, 251)), replace=False)).astype(np.int64)
        else:
            m = int(rng.integers(1, 301)) if i % 4 else int(rng.integers(1, 6))
            ids = np.sort(rng.choice(2000, m, replace=False)).astype(np.int64)
        m = ids.size
        vals = (rng.integers(1, 9, size=m) * 0.3).astype(np.float32)  # (0.3 is no float32 number: the chains round)
        vals[rng.random(m) < 0.05] = 0.0
        rows.append((ids, vals))
    indptr, indices, values = csr(rows)
    got = ctx.knn_sparse(indptr, indices, values, F, 20, metric=WJ)
    t = ctx.last_knn_trace()
    assert 0 < t["range_queries"] < n, t  # (tables on either side of SP_LIMIT)
    _same(got, model.knn_all(indptr, indices, values, F, 20))


# ---- 5. range split ---------------------------------------------------------------------------------------------------
def _heavy_rows(n, seed):
    """Feature 0 in every row, a few medium features (df ~ n / 50) and private-ish light ones."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        ids = {0, 1 + int(rng.integers(0, 50)), 100 + int(rng.integers(0, 5000))}
        if i % 3 == 0:
            ids.add(6000 + int(rng.integers(0, 100000)))
        ids = np.array(sorted(ids), np.int64)
        vals = (rng.integers(1, 8, size=ids.size) * 0.25).astype(np.float32)
        if i % 11 == 0:
            vals[-1] = 0.0  # (feature 0 stays present in every row)
        rows.append((ids, vals))
    return csr(rows)


def test_heavy_postings_take_the_range_split(ctx):
    n, F, k = 20000, 1 << 24, 20
    indptr, indices, values = _heavy_rows(n, seed=5)
    got = ctx.knn_sparse(indptr, indices, values, F, k, metric=WJ)
    t = ctx.last_knn_trace()
    assert t["kind"] == "sparse" and t["range_queries"] > 0 and t["range_chunks"] > 1, t
    rng = np.random.default_rng(3)
    rows = np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), rng.choice(n, 40, replace=False)]))
    _same_rows(got, rows, model.knn_rows(indptr, indices, values, F, k, rows))


# ---- 6. values all 1 are the Jaccard search ---------------------------------------------------------------------------
def test_all_ones_values_give_the_jaccard_bits(ctx):
    F, k = 1 << 25, 20
    indptr, indices, values = weighted_rows(3000, seed=9, n_ids=300)
    want = ctx.knn_sparse(indptr, indices, None, F, k, metric="jaccard")
    _same(ctx.knn_sparse(indptr, indices, None, F, k, metric=WJ), want)
    _same(ctx.knn_sparse(indptr, indices, np.ones(indices.size, np.float32), F, k, metric=WJ), want)
    some = (values != 0).astype(np.float32)  # (stored zeros among the ones)
    _same(ctx.knn_sparse(indptr, indices, some, F, k, metric=WJ),
          ctx.knn_sparse(indptr, indices, some, F, k, metric="jaccard"))
    weighted = ctx.knn_sparse(indptr, indices, values, F, k, metric=WJ)
    assert np.any(weighted[0] != want[0])  # (the weights are not ignored)


# ---- 7. the index and the ranks of a world ----------------------------------------------------------------------------
def test_the_index_in_row_ranges_and_three_ranks(ctx):
    from fedrann_amd.distributed import sparse_knn_rank
    F = 1 << 25
    indptr, indices, values = weighted_rows(3000, seed=1702, n_ids=300)
    n = indptr.size - 1
    A = model.masses(indptr, indices, values)
    ranges = [(0, 1), (1, 64), (64, 65), (65, 97), (97, 98), (98, 2999), (2999, 3000)]  # (row 97 is an empty row)
    whole = {k: ctx.knn_sparse(indptr, indices, values, F, k, metric=WJ) for k in (20, 128)}
    with ctx.sparse_index(indptr, indices, values, F, metric=WJ) as index:
        info = index.info()
        assert info["metric"] == WJ and info["n"] == n and info["zero_rows"] == int(np.sum(A == 0)) > 0, info
        assert info["postings"] == int(np.sum(values > 0)), info
        for k in (20, 128):
            got = [index.search(k, lo, hi) for lo, hi in ranges]
            _same((np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])), whole[k])
        index.search(20, 97, 98)
        assert ctx.last_knn_trace()["zero_queries"] == 1 and A[97] == 0
    parts = [sparse_knn_rank(ctx, indptr, indices, values, F, 20, rank, 3, metric=WJ, block_rows=700)
             for rank in range(3)]
    assert [p[0] for p in parts] == [0] + [p[1] for p in parts[:-1]] and parts[-1][1] == n
    _same((np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])), whole[20])


# ---- 8. arguments -----------------------------------------------------------------------------------------------------
def _raw_call(ctx, metric, indptr, indices, values, F, k):
    n = indptr.size - 1
    idx = np.empty((n, k), np.int32)
    dist = np.empty((n, k), np.float32)
    vp = ctypes.c_void_p
    rc = ctx._L.fdr_knn_sparse_metric(ctx._h, metric, n, F, vp(indptr.ctypes.data), vp(indices.ctypes.data),
                                      vp(values.ctypes.data) if values is not None else None, k,
                                      vp(idx.ctypes.data), vp(dist.ctypes.data))
    return rc, idx, dist


def test_argument_errors(ctx):
    F = 1 << 20
    code = _lib.METRIC_WEIGHTED_JACCARD
    indptr, indices, values = weighted_rows(200, seed=2, F=F, n_ids=128)
    E_ARG = -1
    two = int(np.flatnonzero(np.diff(indptr) >= 2)[0])
    a = int(indptr[two])
    for v, word in ((-0.37, b"negative"), (np.nan, b"finite"), (np.inf, b"finite")):
        bad = values.copy()
        bad[a] = v
        with pytest.raises(ValueError):
            ctx.knn_sparse(indptr, indices, bad, F, 5, metric=WJ)
        assert _raw_call(ctx, code, indptr, indices, bad, F, 5)[0] == E_ARG
        assert word in ctx._L.fdr_last_error(), ctx._L.fdr_last_error()
    bad = values.copy()
    bad[a] = bad[a + 1] = 3e38  # finite values, a mass chain that overflows
    with pytest.raises(ValueError):
        ctx.knn_sparse(indptr, indices, bad, F, 5, metric=WJ)
    assert _raw_call(ctx, code, indptr, indices, bad, F, 5)[0] == E_ARG
    assert b"finite" in ctx._L.fdr_last_error() and b"sum" in ctx._L.fdr_last_error()
    with pytest.raises(_lib.FedrannHipError):  # (the index build refuses it too, and leaves no index)
        ctx._check(ctx._L.fdr_sparse_index_build(ctx._h, code, 200, F, ctypes.c_void_p(indptr.ctypes.data),
                                                 ctypes.c_void_p(indices.ctypes.data),
                                                 ctypes.c_void_p(bad.ctypes.data)), "fdr_sparse_index_build")
    assert ctx._L.fdr_sparse_index_info(ctx._h, None, None, None, None, None) != 0
    desc = indices.copy()
    desc[a], desc[a + 1] = indices[a + 1], indices[a]
    with pytest.raises((ValueError, _lib.FedrannHipError)):
        ctx.knn_sparse(indptr, desc, values, F, 5, metric=WJ)
    assert _raw_call(ctx, code, indptr, desc, values, F, 5)[0] == E_ARG
    big = indices.copy()
    big[indptr[two + 1] - 1] = F
    with pytest.raises((ValueError, _lib.FedrannHipError)):
        ctx.knn_sparse(indptr, big, values, F, 5, metric=WJ)
    assert _raw_call(ctx, code, indptr, big, values, F, 5)[0] == E_ARG
    with pytest.raises((ValueError, _lib.FedrannHipError)):
        ctx.knn_sparse(indptr[:4], indices[:indptr[3]], values[:indptr[3]], F, 5, metric=WJ)  # k > n
    assert _raw_call(ctx, code, indptr[:4].copy(), indices, values, F, 5)[0] == E_ARG
    got = ctx.knn_sparse(indptr, indices, values, F, 5, metric=WJ)  # (the context is fine afterwards)
    _same(got, model.knn_all(indptr, indices, values, F, 5))


# ---- 9. NNDescent_ava(metric="weighted_jaccard") --------------------------------------------------------------------
def test_nndescent_weighted_jaccard_sparse_and_dense_input(ctx):
    from fedrann_amd.nearest_neighbors import NNDescent_ava
    indptr, indices, values = weighted_rows(2000, seed=22, F=1024, n_ids=1024)
    A = sp.csr_matrix((values, indices, indptr), shape=(2000, 1024))
    want = model.knn_all(indptr, indices, values, 1024, 20)
    got = NNDescent_ava().get_neighbors(A, metric=WJ, index_n_neighbors=20, context=ctx, verbose=False)
    assert ctx.last_knn_trace()["kind"] == "sparse"
    _same(got, want)
    got = NNDescent_ava().get_neighbors(A.toarray(), metric=WJ, index_n_neighbors=20, context=ctx, verbose=False)
    assert ctx.last_knn_trace()["kind"] == "sparse"
    _same(got, want)
    with pytest.raises(ValueError, match="cosine.*jaccard"):
        NNDescent_ava().get_neighbors(A, metric="euclidean", index_n_neighbors=20, context=ctx, verbose=False)


# ---- 10. the command line -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads():
    from fedrann_amd.synth import synth
    return synth(3000, seed=44, doubling=True)


@pytest.mark.parametrize("clamp", [False, True])
def test_cli_no_projection_metric_weighted_jaccard(ctx, reads, tmp_path, clamp):
    from fedrann_amd.__main__ import write_overlaps
    from fedrann_amd.feature_extraction import save_feature_matrix_npz
    from fedrann_amd.precompute import idf_weights
    s = reads
    F = s["n_features"]
    counts = s["counts"].copy()
    if clamp:
        counts[int(np.argmax(counts))] = F + 7  # ln(F / count) < 0 for the most frequent k-mer and its complement
    fm, cnt = str(tmp_path / "feature_matrix.npz"), str(tmp_path / "counts.npy")
    save_feature_matrix_npz(fm, s["indptr"], s["indices"], F)
    np.save(cnt, counts)
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "fedrann_amd", "-o", str(out), "--feature-matrix", fm, "--kmer-counts",
                        cnt, "--no-projection", "--no-projection-metric", WJ, "--nndescent-n-neighbors", "20"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    idf = idf_weights(counts, F)
    negative = int(np.sum(idf < 0))
    assert negative == (2 if clamp else 0)
    assert "metric = weighted_jaccard" in r.stderr and "%d of %d features have a negative IDF" % (negative, F) in r.stderr
    w = np.maximum(idf, np.float32(0))
    idx, dist = ctx.knn_sparse(s["indptr"], s["indices"], w[s["indices"]], F, 20, metric=WJ)
    want = tmp_path / "want.tsv"
    n = s["indptr"].size - 1
    write_overlaps(str(want), idx, dist, ["row_%d" % i for i in range(n)], [0] * n)  # (no --read-names)
    assert (out / "overlaps.tsv").read_bytes() == want.read_bytes()
    rows = np.random.default_rng(12).choice(n, 60, replace=False)
    _same_rows((idx, dist), rows, model.knn_rows(s["indptr"], s["indices"], w[s["indices"]], F, 20, rows))
    if clamp:
        assert np.any(idf[s["indices"]] < 0)  # (the clamped feature occurs in the rows)
        cos_idx, _ = ctx.knn_sparse(s["indptr"], s["indices"], idf[s["indices"]], F, 20)  # (cosine keeps the sign)
        assert np.any(cos_idx != idx)
