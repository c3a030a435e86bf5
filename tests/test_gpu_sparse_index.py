"""The sparse index built once and searched by row ranges (fdr_sparse_index_build / _search / _info / _free,
Context.sparse_index, distributed.sparse_knn_rank): every partition of the rows gives the whole call's bits (the whole
call is pinned to the oracle and to the Jaccard model by test_gpu_sparse_knn / test_gpu_sparse_jaccard), range-split
queries inside a range, n == k, the index across other calls on the context, and three ranks on one GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _jaccard_model as model
from fedrann_amd import _lib
from test_gpu_sparse_knn import _check_queries, _hard_rows, _heavy_rows, _same, _synth_idf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F = 1 << 25
E_ARG, E_STATE = -1, -5
RANGES = [(0, 1), (1, 64), (64, 65), (65, 97), (97, 98), (98, 2999), (2999, 3000)]  # (row 97 is an empty row)


def _values(values, metric):
    return values if metric == "cosine" else None


def _zero_rows(indptr, values):
    """bool [n]: the rows without a value other than 0 (values=None: the empty rows)."""
    if values is None:
        return np.diff(indptr) == 0
    return np.array([not np.any(values[indptr[r]:indptr[r + 1]]) for r in range(indptr.size - 1)])


def _pieces(index, k, ranges):
    got = [index.search(k, lo, hi) for lo, hi in ranges]
    for (lo, hi), (i, d) in zip(ranges, got):
        assert i.shape == d.shape == (hi - lo, k) and i.dtype == np.int32 and d.dtype == np.float32
    return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])


# ---- 1. a partition equals the whole call -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hard():
    indptr, indices, values, _ = _hard_rows(3000, seed=1702, n_ids=300)
    assert indptr[98] == indptr[97] and np.any(values == 0)
    return indptr, indices, values


@pytest.mark.parametrize("metric", ["cosine", "jaccard"])
@pytest.mark.parametrize("k", [1, 20, 128])
def test_a_partition_equals_the_whole_call(ctx, hard, metric, k):
    indptr, indices, values = hard
    v = _values(values, metric)
    whole = ctx.knn_sparse(indptr, indices, v, F, k, metric=metric)
    with ctx.sparse_index(indptr, indices, v, F, metric=metric) as index:
        _same(_pieces(index, k, RANGES), whole)
        t = ctx.last_knn_trace()  # (of the last range)
        assert t["kind"] == "sparse" and t["queries"] == 1 and t["targets"] == 3000 and t["k"] == k, t
        zero = _zero_rows(indptr, v)
        for lo, hi in ((97, 98), (98, 194), (0, 3000)):  # (rows of stored zeros only: zero rows of the cosine search)
            index.search(k, lo, hi)
            assert ctx.last_knn_trace()["zero_queries"] == int(zero[lo:hi].sum()), (lo, hi)
        assert zero[97] and zero[98:194].sum() < zero.sum()


# ---- 2. heavy queries inside and outside the range --------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "jaccard"])
def test_range_split_queries_of_a_row_range(ctx, oracle, metric):
    n, Fh, k = 3000, 1 << 24, 20
    indptr, indices, values = _heavy_rows(n, seed=6)
    with ctx.sparse_index(indptr, indices, values, Fh, metric=metric) as index:
        part = index.search(k, 1000, 1300)
        t = ctx.last_knn_trace()
        assert t["kind"] == "sparse" and t["queries"] == 300 and t["targets"] == 3000, t
        assert 0 < t["range_queries"] <= 300 and t["range_chunks"] == 6, t
        full = index.search(k)
        t = ctx.last_knn_trace()
        assert t["queries"] == 3000 and t["range_queries"] > 300, t
    _same(part, (full[0][1000:1300], full[1][1000:1300]))
    rows = np.unique(np.concatenate([[1000, 1299], np.random.default_rng(4).choice(np.arange(1001, 1299), 10,
                                                                                   replace=False)]))
    if metric == "cosine":
        got = (np.full((n, k), -1, np.int32), np.zeros((n, k), np.float32))
        got[0][1000:1300], got[1][1000:1300] = part
        _check_queries(oracle, indptr, indices, values, Fh, k, rows, got)
    else:
        _same((part[0][rows - 1000], part[1][rows - 1000]), model.knn_rows(indptr, indices, values, Fh, k, rows))


# ---- 3. n == k and tiny sets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "jaccard"])
@pytest.mark.parametrize("n", [1, 5, 64])
def test_n_equals_k_row_by_row(ctx, n, metric):
    indptr, indices, values, _ = _hard_rows(n, seed=n, F=1 << 24, n_ids=128, per=(1, 4))
    whole = ctx.knn_sparse(indptr, indices, values, 1 << 24, n, metric=metric)
    with ctx.sparse_index(indptr, indices, values, 1 << 24, metric=metric) as index:
        _same(_pieces(index, n, [(r, r + 1) for r in range(n)]), whole)
        assert _raw_search(ctx, n + 1, 0, n)[0] == E_ARG  # k > n


# ---- 4. the index persists --------------------------------------------------------------------------------------------
def test_the_index_survives_other_calls(ctx, hard):
    indptr, indices, values = hard
    want20 = ctx.knn_sparse(indptr, indices, values, F, 20)
    want50 = ctx.knn_sparse(indptr, indices, values, F, 50)
    index = ctx.sparse_index(indptr, indices, values, F)
    info = index.info()
    zero_rows = int(_zero_rows(indptr, values).sum())
    assert info["metric"] == "cosine" and info["n"] == 3000 and info["zero_rows"] == zero_rows > 0, info
    assert info["postings"] == int(np.count_nonzero(values)) and info["device_bytes"] >= 20 * indices.size, info
    _same(index.search(20), want20)
    E = np.random.default_rng(12).standard_normal((700, 64)).astype(np.float32)
    E[::9] = 0.0  # (zero rows: the dense call writes its own zero flags)
    ctx.knn(E, 10)
    assert ctx.last_knn_trace()["kind"] != "sparse"
    _same(index.search(50), want50)
    _same(index.search(20), want20)
    assert index.info() == info
    out = (np.empty((300, 20), np.int32), np.empty((300, 20), np.float32))
    got = index.search(20, 500, 800, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    _same(out, (want20[0][500:800], want20[1][500:800]))
    index.close()
    with pytest.raises(_lib.FedrannHipError, match="closed"):
        index.search(20)
    index.close()  # (twice is fine)


def test_a_second_index_makes_the_first_raise(ctx, hard):
    indptr, indices, values = hard
    small = _hard_rows(64, seed=3, F=1 << 24, n_ids=128, per=(1, 4))[:3]
    first = ctx.sparse_index(indptr, indices, values, F)
    with ctx.sparse_index(*small, 1 << 24, metric="jaccard") as second:
        with pytest.raises(_lib.FedrannHipError, match="another sparse index"):
            first.search(20)
        with pytest.raises(_lib.FedrannHipError, match="another sparse index"):
            first.info()
        first.close()  # (must not free the second one)
        assert second.info()["n"] == 64 and second.info()["metric"] == "jaccard"
        got = second.search(5)
    _same(got, ctx.knn_sparse(*small, 1 << 24, 5, metric="jaccard"))
    third = ctx.sparse_index(*small, 1 << 24)
    ctx.knn_sparse(indptr, indices, values, F, 20)  # (the whole call builds the context's index anew)
    with pytest.raises(_lib.FedrannHipError, match="another sparse index"):
        third.search(5)


def _raw_build(ctx, metric, indptr, indices, values, n_features):
    vp = ctypes.c_void_p
    return ctx._L.fdr_sparse_index_build(ctx._h, metric, indptr.size - 1, n_features, vp(indptr.ctypes.data),
                                         vp(indices.ctypes.data), vp(values.ctypes.data))


def _raw_search(ctx, k, lo, hi):
    idx, dist = np.empty((hi - lo, k), np.int32), np.empty((hi - lo, k), np.float32)
    vp = ctypes.c_void_p
    return ctx._L.fdr_sparse_index_search(ctx._h, k, lo, hi, vp(idx.ctypes.data), vp(dist.ctypes.data)), idx, dist


@pytest.mark.parametrize("metric", [_lib.METRIC_COSINE, _lib.METRIC_JACCARD])
def test_a_refused_build_leaves_no_index(ctx, metric):
    Fs = 1 << 20
    indptr, indices, values, _ = _hard_rows(200, seed=2, F=Fs, n_ids=128)
    two = np.flatnonzero(np.diff(indptr) >= 2)[0]
    a = int(indptr[two])
    big = indices.copy()
    big[indptr[two + 1] - 1] = Fs  # an id >= F
    desc = indices.copy()
    desc[a], desc[a + 1] = indices[a + 1], indices[a]  # descending ids
    nan = values.copy()
    nan[a] = np.nan
    for ix, v in ((big, values), (desc, values), (indices, nan)):
        assert _raw_build(ctx, metric, indptr, indices, values, Fs) == 0
        rc, idx, dist = _raw_search(ctx, 5, 0, 200)
        assert rc == 0
        assert _raw_build(ctx, metric, indptr, ix, v, Fs) == E_ARG
        assert _raw_search(ctx, 5, 0, 200)[0] == E_STATE
        assert ctx._L.fdr_sparse_index_info(ctx._h, None, None, None, None, None) == E_STATE
    assert _raw_build(ctx, 7, indptr, indices, values, Fs) == E_ARG and b"metric" in ctx._L.fdr_last_error()
    assert _raw_build(ctx, metric, indptr, indices, values, Fs) == 0
    room = np.empty(256 * 128, np.int32)  # (enough for any of the refused shapes)
    buf = ctypes.c_void_p(room.ctypes.data)
    for k, lo, hi in ((0, 0, 200), (129, 0, 200), (-3, 0, 200), (5, -1, 3), (5, 4, 3), (5, 0, 201), (5, 200, 201)):
        assert ctx._L.fdr_sparse_index_search(ctx._h, k, lo, hi, buf, buf) == E_ARG, (k, lo, hi)
    assert ctx._L.fdr_sparse_index_search(ctx._h, 5, 0, 3, None, None) == E_ARG  # null results of a non-empty range
    rc, idx2, dist2 = _raw_search(ctx, 5, 0, 200)  # (the index is fine after refused searches)
    assert rc == 0
    _same((idx2, dist2), (idx, dist))
    assert ctx._L.fdr_sparse_index_free(ctx._h) == 0
    assert _raw_search(ctx, 5, 0, 200)[0] == E_STATE
    assert ctx._L.fdr_sparse_index_free(ctx._h) == 0  # (nothing to free: fine)


def test_a_refused_whole_call_leaves_no_index(ctx):
    """fdr_knn_sparse replaces the context's index, so where it is refused, before its build too, there is none."""
    Fs = 1 << 20
    indptr, indices, values, _ = _hard_rows(200, seed=2, F=Fs, n_ids=128)
    vp = ctypes.c_void_p
    room = np.empty(200 * 128, np.int32)
    for k in (0, 129, 201):
        assert _raw_build(ctx, _lib.METRIC_COSINE, indptr, indices, values, Fs) == 0
        assert _raw_search(ctx, 5, 0, 200)[0] == 0
        rc = ctx._L.fdr_knn_sparse(ctx._h, 200, Fs, vp(indptr.ctypes.data), vp(indices.ctypes.data),
                                   vp(values.ctypes.data), k, vp(room.ctypes.data), vp(room.ctypes.data))
        assert rc == E_ARG, k
        assert _raw_search(ctx, 5, 0, 200)[0] == E_STATE, k


# ---- 5. the empty range -----------------------------------------------------------------------------------------------
def test_an_empty_range(ctx, hard):
    indptr, indices, values = hard
    with ctx.sparse_index(indptr, indices, values, F) as index:
        for at in (0, 97, 3000):
            idx, dist = index.search(20, at, at)
            assert idx.shape == dist.shape == (0, 20) and idx.dtype == np.int32 and dist.dtype == np.float32
        t = ctx.last_knn_trace()
        assert t["kind"] == "sparse" and t["queries"] == 0 and t["targets"] == 3000, t


# ---- 6. three ranks on GPU 0 ------------------------------------------------------------------------------------------
def test_three_ranks_tile_the_whole_call(ctx, tmp_path):
    R, k, world = 3000, 20, 3
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_gpu_sparse_rank_worker.py"), str(tmp_path), str(R),
                               str(k), "700", str(rank), str(world)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for rank in range(world)]
    try:
        outs = [p.communicate(timeout=300)[0].decode(errors="replace") for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    indptr, indices, values, Fs = _synth_idf(R)
    n = indptr.size - 1
    want = ctx.knn_sparse(indptr, indices, values, Fs, k)
    rows, idx, dist = 0, [], []
    for rank in range(world):
        z = np.load(os.path.join(str(tmp_path), "rank%d.npz" % rank))
        lo, hi = int(z["lo"]), int(z["hi"])
        assert lo == rows and z["idx"].shape == z["dist"].shape == (hi - lo, k)
        assert int(z["targets"]) == n and 0 < int(z["queries"]) <= 700
        rows = hi
        idx.append(z["idx"])
        dist.append(z["dist"])
    assert rows == n
    _same((np.concatenate(idx), np.concatenate(dist)), want)
