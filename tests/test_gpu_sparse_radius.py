"""Radius search on the sparse index (fdr_sparse_index_radius_search / _radius_query / _radius_fetch): every index row
within a distance bound, against the numpy models of tests/_radius_model.py.  Every comparison is exact: equal indptr,
equal indices, equal distance bit patterns.  The inputs are the generators of test_gpu_sparse_knn / test_gpu_sparse_query;
the hit counts asserted below were computed on the CPU from the models with those generators and seeds, so that no
test can pass on empty rows."""
import ctypes

import numpy as np
import pytest

import _radius_model as rmodel
from _weighted_rows import csr as rows_csr
from _weighted_rows import weighted_rows
from fedrann_amd import _lib
from test_gpu_sparse_knn import _hard_rows, _heavy_rows, _same
from test_gpu_sparse_query import F, METRICS, _cut, _external, _own, _rows_of, _zero_rows

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5
RADII = (0.0, 0.5, 0.9, 0.97)
TOTALS = {"cosine": (785, 1296, 22494, 39184), "jaccard": (812, 898, 20507, 86100),
          "weighted_jaccard": (767, 832, 13045, 63486)}
MAX_ROW = {"cosine": 284, "jaccard": 671, "weighted_jaccard": 462}  # the longest row at r = 0.97
vp = ctypes.c_void_p


def _keys(idx, dist):
    return (dist.view(np.uint32).astype(np.int64) << 32) | idx.astype(np.int64)


def _row(res, i):
    return res[1][res[0][i]:res[0][i + 1]], res[2][res[0][i]:res[0][i + 1]]


# ---- 1. model parity, all three metrics -------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=METRICS)
def external(request, oracle):
    metric = request.param
    targets, queries, _ = _external(metric)
    ones = (queries[0], queries[1], None)
    return metric, targets, queries, ones, rmodel.model(metric, oracle, targets, queries, F), \
        rmodel.model(metric, oracle, targets, ones, F)


def test_external_queries_match_the_model(ctx, external):
    metric, targets, queries, ones, want, want_ones = external
    nq = queries[0].size - 1
    with ctx.sparse_index(*targets, F, metric=metric) as index:
        for r, total in zip(RADII, TOTALS[metric]):
            got = index.radius_query(*queries, r)
            t = ctx.last_knn_trace()
            print("%s r = %g: %d hits, longest row %d, %d range queries"
                  % (metric, r, got[0][-1], np.diff(got[0]).max(), t["range_queries"]))
            rmodel.same(got, want(r))
            assert got[0][-1] == total
            assert t["kind"] == "sparse" and t["k"] == 0 and t["queries"] == nq == 400 and t["targets"] == 3000, t
            assert t["zero_queries"] == int(_zero_rows(queries[0], queries[2], metric).sum()) > 0, t
            if r == 0.97:
                assert np.diff(got[0]).max() == MAX_ROW[metric]
            if metric != "cosine":  # (these fixtures cross the heavy path: queries with more than SP_LIMIT targets)
                assert t["range_queries"] > 0 and t["range_chunks"] == 6, t
            rmodel.same(index.radius_query(*queries, r, block_rows=150), want(r))
            # queries without values (every stored entry 1) against the index built with values
            rmodel.same(index.radius_query(*ones, r), want_ones(r))


# ---- 2. heavy segments: a heavy query's hits across its ranges --------------------------------------------------------
def test_heavy_segments_are_ordered_across_the_ranges(ctx):
    Fh = 1 << 24
    targets = _heavy_rows(3000, seed=6)
    queries = _heavy_rows(300, seed=7)
    sample = _cut(*queries, 0, 40)
    D = rmodel.distances("jaccard", targets, sample, Fh)
    with ctx.sparse_index(*targets, Fh, metric="jaccard") as index:
        for r, lo, hi, total in ((0.7, 40, 80, 2386), (0.85, 2012, 3000, 106261)):
            got = index.radius_query(*sample, r)
            t = ctx.last_knn_trace()
            counts = np.diff(got[0])
            print("r = %g: %d hits, %d .. %d per query, %d range queries"
                  % (r, got[0][-1], counts.min(), counts.max(), t["range_queries"]))
            rmodel.same(got, rmodel.rows_within(D, r))
            assert got[0][-1] == total and lo <= counts.min() and counts.max() <= hi
            assert t["range_queries"] > 0 and t["range_chunks"] == 6, t
        first = got
        got = index.radius_query(*queries, 0.85)
        assert got[0][0] == 0 and np.all(np.diff(got[0]) >= 0) and got[0][-1] == got[1].size == got[2].size
        keys = _keys(got[1], got[2])
        inner = np.ones(keys.size, bool)
        inner[got[0][1:-1][got[0][1:-1] < keys.size]] = False  # (a row's first key follows another row's last)
        assert np.all((np.diff(keys) > 0) | ~inner[1:])
        n40 = first[0][-1]
        assert np.array_equal(got[0][:41], first[0]) and np.array_equal(got[1][:n40], first[1]) \
            and np.array_equal(got[2][:n40].view(np.uint32), first[2].view(np.uint32))


# ---- 3. own rows and the prefix property ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_own_rows_equal_the_query_and_prefix_the_knn_search(ctx, metric):
    indptr, indices, values = _own(metric)
    zero = _zero_rows(indptr, values, metric)
    with ctx.sparse_index(indptr, indices, values, F, metric=metric) as index:
        for lo, hi in ((0, 1), (97, 98), (98, 2999), (2500, 3001)):
            s_idx, s_dist = index.search(128, lo, hi)
            for r in (0.5, 0.9):
                got = index.radius_search(r, lo, hi)
                t = ctx.last_knn_trace()
                assert t["kind"] == "sparse" and t["k"] == 0 and t["queries"] == hi - lo and t["targets"] == 3001, t
                assert t["zero_queries"] == int(zero[lo:hi].sum()), t
                rmodel.same(index.radius_query(*_cut(indptr, indices, values, lo, hi), r), got)
                assert got[0][-1] > hi - lo or hi - lo == 1
                for i in range(hi - lo):
                    gi, gd = _row(got, i)
                    keep = s_dist[i] <= np.float32(r)
                    m = min(128, gi.size)
                    assert int(keep.sum()) == m, (lo + i, r)
                    assert np.array_equal(gi[:m], s_idx[i][keep]) and \
                        np.array_equal(gd[:m].view(np.uint32), s_dist[i][keep].view(np.uint32)), (lo + i, r)
                    assert lo + i in gi  # self (a zero row is among the zero rows)
                    assert np.all(np.diff(_keys(gi, gd)) > 0) and (gi.size == 0 or gd[-1] <= np.float32(r))


# ---- 4. zero queries --------------------------------------------------------------------------------------------------
ZERO_QUERIES = (np.array([0, 0, 2, 2], np.int64), np.array([0, 3], np.int32), np.array([0.0, -0.0], np.float32))


@pytest.mark.parametrize("metric", METRICS)
def test_zero_queries_get_the_zero_rows(ctx, metric):
    indptr, indices, values = _own(metric)
    zrows = np.flatnonzero(_zero_rows(indptr, values, metric)).astype(np.int32)
    assert zrows.size > 3
    with ctx.sparse_index(indptr, indices, values, F, metric=metric) as index:
        assert index.info()["zero_rows"] == zrows.size
        for r in (0.0, 0.5):
            ip, idx, dist = index.radius_query(*ZERO_QUERIES, r)
            assert ctx.last_knn_trace()["zero_queries"] == 3
            assert np.array_equal(ip, zrows.size * np.arange(4)) and np.array_equal(idx, np.tile(zrows, 3))
            assert np.all(dist.view(np.uint32) == 0)
            # ... and an own zero row at r = 0 too
            z = int(zrows[1])
            ip, idx, dist = index.radius_search(r, z, z + 1)
            assert np.array_equal(idx, zrows) and np.all(dist.view(np.uint32) == 0) and ip[-1] == zrows.size
    h = _heavy_rows(200, seed=8)
    with ctx.sparse_index(*h, 1 << 24, metric=metric) as index:
        assert index.info()["zero_rows"] == 0
        ip, idx, dist = index.radius_query(*ZERO_QUERIES, 0.5)
        assert ctx.last_knn_trace()["zero_queries"] == 3
        assert np.array_equal(ip, np.zeros(4, np.int64)) and idx.size == 0 and dist.size == 0


# ---- 5. small sets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 5, 64])
def test_small_sets(ctx, oracle, n, metric):
    if metric == "weighted_jaccard":
        targets = weighted_rows(n, seed=n, F=1 << 24, n_ids=128, per=(1, 4))
    else:
        targets = _hard_rows(n, seed=n, F=1 << 24, n_ids=128, per=(1, 4))[:3]
    # the four queries of test_k_equals_n_and_fewer_queries_than_k: over ids of the targets, empty, alone with an id
    # of its own, and a copy of the last target row
    first = np.unique(targets[1]).astype(np.int64)[:3]
    queries = rows_csr([(first, (0.37 * (1 + np.arange(first.size))).astype(np.float32)),
                        (np.zeros(0, np.int64), np.zeros(0, np.float32)),
                        (np.array([(1 << 24) - 1], np.int64), np.array([1.5], np.float32)),
                        _rows_of(*targets)[n - 1]])
    want = rmodel.model(metric, oracle, targets, queries, 1 << 24)
    with ctx.sparse_index(*targets, 1 << 24, metric=metric) as index:
        for r in RADII:
            rmodel.same(index.radius_query(*queries, r), want(r))
            rmodel.same(index.radius_search(r), index.radius_query(*targets, r))
        assert index.radius_search(0.5)[0][-1] >= n  # (self, or the zero rows)
        ip, idx, dist = index.radius_query(np.zeros(1, np.int64), np.zeros(0, np.int32), None, 0.5)
        assert np.array_equal(ip, [0]) and ip.dtype == np.int64 and idx.shape == dist.shape == (0,)
        t = ctx.last_knn_trace()
        assert t["kind"] == "sparse" and t["queries"] == 0 and t["targets"] == n and t["k"] == 0, t
        ip, idx, dist = index.radius_search(0.5, n, n)
        assert np.array_equal(ip, [0]) and idx.size == 0


# ---- 6. the cap -------------------------------------------------------------------------------------------------------
def _raw_radius_search(ctx, r, lo, hi, max_hits):
    indptr = np.full(hi - lo + 1, -7, np.int64)
    rc = ctx._L.fdr_sparse_index_radius_search(ctx._h, ctypes.c_float(r), lo, hi, max_hits, vp(indptr.ctypes.data))
    return rc, indptr


def _raw_fetch(ctx, hits):
    idx, dist = np.empty(max(hits, 1), np.int32), np.empty(max(hits, 1), np.float32)
    return ctx._L.fdr_sparse_index_radius_fetch(ctx._h, hits, vp(idx.ctypes.data), vp(dist.ctypes.data)), idx, dist


@pytest.mark.parametrize("metric", ["cosine", "jaccard"])
def test_the_cap_refuses_with_the_counts_and_the_wrapper_cuts_the_block(ctx, metric):
    indptr, indices, values = _own(metric)
    with ctx.sparse_index(indptr, indices, values, F, metric=metric) as index:
        s20 = index.search(20)
        whole = index.radius_search(0.9)
        total = int(whole[0][-1])
        counts = np.diff(whole[0])
        assert total > 3001 and counts.max() > 20
        rc, ip = _raw_radius_search(ctx, 0.9, 0, 3001, total - 1)
        msg = ctx._L.fdr_last_error().decode()
        assert rc == E_ARG and str(total) in msg and str(total - 1) in msg and "max_hits" in msg, msg
        assert np.array_equal(ip, whole[0])  # the one refusal that writes its output
        assert _raw_fetch(ctx, total)[0] == E_STATE and _raw_fetch(ctx, 0)[0] == E_STATE
        _same(index.search(20), s20)
        rc, ip = _raw_radius_search(ctx, 0.9, 0, 3001, total)  # exactly the cap: fine
        assert rc == 0 and np.array_equal(ip, whole[0])
        rc, idx, dist = _raw_fetch(ctx, total)
        assert rc == 0 and np.array_equal(idx, whole[1]) and np.array_equal(dist.view(np.uint32), whole[2].view(np.uint32))
        for cap in (total - 1, total // 7, int(counts.max())):
            rmodel.same(index.radius_search(0.9, max_hits=cap), whole)
            rmodel.same(index.radius_query(indptr, indices, values, 0.9, max_hits=cap), whole)
        rmodel.same(index.radius_query(indptr, indices, values, 0.9, max_hits=total // 3, block_rows=1000), whole)
        q = int(np.argmax(counts))
        with pytest.raises(_lib.FedrannHipError, match="query %d alone has %d hits" % (q, counts[q])):
            index.radius_search(0.9, max_hits=int(counts.max()) - 1)
        q = 100 + int(np.argmax(counts[100:]))  # (the message numbers the index's rows, not the range's)
        with pytest.raises(_lib.FedrannHipError, match="query %d alone" % q):
            index.radius_search(0.9, 100, 3001, max_hits=int(counts[q]) - 1)
        _same(index.search(20), s20)
        for bad in (0, 1 << 31, -5):
            assert _raw_radius_search(ctx, 0.9, 0, 10, bad)[0] == E_ARG


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def _raw_radius_query(ctx, r, indptr, indices, values, max_hits=1 << 20):
    out = np.full(indptr.size, -7, np.int64)
    rc = ctx._L.fdr_sparse_index_radius_query(ctx._h, ctypes.c_float(r), indptr.size - 1, vp(indptr.ctypes.data),
                                              vp(indices.ctypes.data),
                                              None if values is None else vp(values.ctypes.data), max_hits,
                                              vp(out.ctypes.data))
    return rc, out


def test_refusals_leave_the_index_and_name_the_cause(ctx):
    Fs, n = 1 << 20, 200
    indptr, indices, values, _ = _hard_rows(n, seed=2, F=Fs, n_ids=128)
    assert ctx._L.fdr_sparse_index_free(ctx._h) == 0
    assert _raw_radius_search(ctx, 0.5, 0, n, 1 << 20)[0] == E_STATE
    assert b"no sparse index" in ctx._L.fdr_last_error()
    assert _raw_radius_query(ctx, 0.5, indptr, indices, values)[0] == E_STATE
    assert _raw_fetch(ctx, 0)[0] == E_STATE
    with ctx.sparse_index(indptr, indices, values, Fs, metric="jaccard") as index:
        s5 = index.search(5)
        before = index.info()["device_bytes"]
        for r in (float("nan"), -0.1, 1.0, float("inf")):
            assert _raw_radius_search(ctx, r, 0, n, 1 << 20)[0] == E_ARG, r
            assert b"[0, 1)" in ctx._L.fdr_last_error()
            assert _raw_radius_query(ctx, r, indptr, indices, values)[0] == E_ARG, r
            with pytest.raises(ValueError, match="radius"):
                index.radius_search(r)
            with pytest.raises(ValueError, match="radius"):
                index.radius_query(indptr, indices, values, r)
        assert _raw_radius_search(ctx, 1.0, 0, n, 1 << 20)[0] == E_ARG
        msg = ctx._L.fdr_last_error().decode()
        assert "every row is within 1" in msg and "fdr_sparse_index_search" in msg, msg
        for lo, hi in ((-1, 5), (5, 4), (0, n + 1)):
            assert _raw_radius_search(ctx, 0.5, lo, hi, 1 << 20)[0] == E_ARG
        # a held result, a wrong count, and an intervening search
        rc, ip = _raw_radius_search(ctx, 0.5, 0, n, 1 << 20)
        total = int(ip[-1])
        assert rc == 0 and total >= n - int(np.sum(_zero_rows(indptr, values, "jaccard"))) > 0
        assert _raw_fetch(ctx, total + 1)[0] == E_ARG and _raw_fetch(ctx, total - 1)[0] == E_ARG
        assert _raw_fetch(ctx, total)[0] == 0
        _same(index.search(5), s5)
        assert _raw_fetch(ctx, total)[0] == E_STATE
        assert b"no radius result" in ctx._L.fdr_last_error()
        # a query row with descending ids: the message of the k-NN query, and the index intact
        two = np.flatnonzero(np.diff(indptr) >= 2)[0]
        a = int(indptr[two])
        desc = indices.copy()
        desc[a], desc[a + 1] = indices[a + 1], indices[a]
        rc, _ = _raw_radius_query(ctx, 0.5, indptr, desc, values)
        assert rc == E_ARG and b"strictly ascending inside a row" in ctx._L.fdr_last_error()
        assert _raw_fetch(ctx, 0)[0] == E_STATE
        big = indices.copy()
        big[a] = Fs
        rc, _ = _raw_radius_query(ctx, 0.5, indptr, big, values)
        assert rc == E_ARG and b"outside [0," in ctx._L.fdr_last_error()
        _same(index.search(5), s5)
        with pytest.raises(ValueError, match="ascending"):
            index.radius_query(indptr, desc, values, 0.5)
        with pytest.raises(ValueError, match="block_rows"):
            index.radius_query(indptr, indices, values, 0.5, block_rows=0)
        with pytest.raises(TypeError):
            index.radius_query(indptr, indices.astype(np.int64), values, 0.5)
        with pytest.raises(ValueError, match="lo"):
            index.radius_search(0.5, 5, 4)
        index.radius_search(0.9)
        assert index.info()["device_bytes"] > before
    with pytest.raises(_lib.FedrannHipError, match="closed"):
        index.radius_search(0.5)
    with pytest.raises(_lib.FedrannHipError, match="closed"):
        index.radius_query(indptr, indices, values, 0.5)
