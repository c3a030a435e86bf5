"""Querying the sparse index with rows that are not in it (fdr_sparse_index_query, SparseIndex.query,
distributed.sparse_knn_target_shard / merge_sparse_topk): the index's own rows as queries give the row-range search's
bits, queries outside the index match models that know nothing of the kernel, the edges, refusals that leave the index
alone, and target shards that compose into the whole call.  Every comparison is exact: equal indices, equal distance
bit patterns."""
import ctypes

import numpy as np
import pytest

import _sparse_query_model as qmodel
from _weighted_rows import csr as rows_csr
from _weighted_rows import weighted_rows
from fedrann_amd import _lib, distributed
from test_gpu_sparse_knn import _hard_rows, _heavy_rows, _row_norms, _same, _synth_idf

pytestmark = pytest.mark.gpu

F = 1 << 25
E_ARG, E_STATE = -1, -5
METRICS = ["cosine", "jaccard", "weighted_jaccard"]
RANGES = [(0, 1), (64, 65), (97, 98), (98, 2999), (0, 3000), (2500, 3001)]  # (row 97 is empty, row 3000 the long one)


def _rows_of(indptr, indices, values):
    return [(indices[indptr[r]:indptr[r + 1]].astype(np.int64), values[indptr[r]:indptr[r + 1]])
            for r in range(indptr.size - 1)]


def _cut(indptr, indices, values, lo, hi):
    """Rows [lo, hi) as a CSR of their own."""
    ip, ix = distributed.local_csr(indptr, indices, lo, hi)
    return ip, ix, (None if values is None else np.ascontiguousarray(values[indptr[lo]:indptr[hi]]))


def _zero_rows(indptr, values, metric):
    """bool [n]: the zero rows of the metric (no value other than +-0)."""
    return np.array([not np.any(values[indptr[r]:indptr[r + 1]] != 0) for r in range(indptr.size - 1)])


# ---- 1. own rows as queries equal the row-range search ----------------------------------------------------------------
def _own(metric):
    if metric == "weighted_jaccard":
        indptr, indices, values = weighted_rows(3000, seed=1702, n_ids=300)
    else:
        indptr, indices, values, _ = _hard_rows(3000, seed=1702, n_ids=300)
    rows = _rows_of(indptr, indices, values)
    assert max(r[0].size for r in rows) <= 64  # (the generators give no row longer than 64 stored entries: append one)
    ids = np.unique(indices)[:150].astype(np.int64)
    vals = (0.37 * (1 + np.arange(150) % 5)).astype(np.float32)
    vals[::17] = 0.0
    rows.append((ids, vals))
    return rows_csr(rows)


@pytest.fixture(scope="module", params=METRICS)
def own(request):
    metric = request.param
    indptr, indices, values = _own(metric)
    assert indptr.size - 1 == 3001 and indptr[98] == indptr[97] and indptr[3001] - indptr[3000] > 64
    zero = _zero_rows(indptr, values, metric)
    stored_zero = np.array([np.any(values[indptr[r]:indptr[r + 1]] == 0) for r in range(3001)])
    for lo, hi in ((98, 2999), (0, 3000), (2500, 3001)):
        assert zero[lo:hi].any() and (stored_zero[lo:hi] & ~zero[lo:hi]).any(), (lo, hi)
    assert zero[97] and not zero[64] and not zero[3000] and stored_zero[3000]
    return metric, indptr, indices, values


@pytest.mark.parametrize("k", [1, 20, 128])
def test_own_rows_as_queries_equal_the_range_search(ctx, own, k):
    metric, indptr, indices, values = own
    with ctx.sparse_index(indptr, indices, values, F, metric=metric) as index:
        assert index.n_features == F and index.n == 3001
        for lo, hi in RANGES:
            want = index.search(k, lo, hi)
            tw = ctx.last_knn_trace()
            got = index.query(*_cut(indptr, indices, values, lo, hi), k)
            tg = ctx.last_knn_trace()
            assert got[0].shape == got[1].shape == (hi - lo, k) and got[0].dtype == np.int32 and got[1].dtype == np.float32
            _same(got, want)
            assert tg == tw, (tg, tw)  # kind, k, queries, targets, zero_queries, range_queries: the same search
        whole = index.search(k)
        for block_rows, hi in ((1, 400), (7, 3001), (1000, 3001)):
            got = index.query(*_cut(indptr, indices, values, 0, hi), k, block_rows=block_rows)
            _same(got, (whole[0][:hi], whole[1][:hi]))
        out = (np.empty((3001, k), np.int32), np.empty((3001, k), np.float32))
        got = index.query(indptr, indices, values, k, out=out, block_rows=np.int64(1500))
        assert got[0] is out[0] and got[1] is out[1]
        _same(out, whole)
        with pytest.raises(ValueError, match="block_rows"):
            index.query(indptr, indices, values, k, block_rows=0)
        with pytest.raises(ValueError, match="out"):
            index.query(indptr, indices, values, k, out=(out[0][:5], out[1][:5]))


# ---- 2. heavy queries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "jaccard"])
def test_heavy_own_rows_take_the_range_split(ctx, metric):
    indptr, indices, values = _heavy_rows(3000, seed=6)
    with ctx.sparse_index(indptr, indices, values, 1 << 24, metric=metric) as index:
        want = index.search(20, 1000, 1300)
        tw = ctx.last_knn_trace()
        got = index.query(*_cut(indptr, indices, values, 1000, 1300), 20)
        t = ctx.last_knn_trace()
    _same(got, want)
    assert t["kind"] == "sparse" and t["queries"] == 300 and t["targets"] == 3000, t
    assert 0 < t["range_queries"] <= 300 and t["range_chunks"] == 6, t
    assert t["range_queries"] == tw["range_queries"]


# ---- 3. queries that are not in the index -----------------------------------------------------------------------------
def _external(metric):
    """(targets, queries, dup): 3000 target rows and 400 query rows over a pool of ids that overlaps the targets' but
    is not equal to it; query row `dup` is a copy of a target row."""
    if metric == "weighted_jaccard":
        targets = weighted_rows(3000, seed=11, n_ids=300)
        q_indptr, q_indices, q_values = weighted_rows(400, seed=12, n_ids=300)
    else:
        targets = _hard_rows(3000, seed=11, n_ids=300)[:3]
        q_indptr, q_indices, q_values = _hard_rows(400, seed=12, n_ids=300)[:3]
    # the queries' distinct ids, renumbered in order: two in three become ids of the targets, the others stay
    rng = np.random.default_rng(13)
    t_ids, q_ids = np.unique(targets[1]), np.unique(q_indices)
    shared = rng.random(q_ids.size) < 2 / 3
    new = np.unique(np.concatenate([rng.choice(t_ids, int(shared.sum()), replace=False), q_ids[~shared]]))
    assert new.size == q_ids.size
    q_indices = new[np.searchsorted(q_ids, q_indices)].astype(np.int32)
    rows = _rows_of(q_indptr, q_indices, q_values)
    t_rows = _rows_of(*targets)
    dup = 50
    rows[dup] = t_rows[20]
    assert t_rows[20][0].size >= 2 and np.any(t_rows[20][1] != 0)
    return targets, rows_csr(rows), dup


def _assert_external_inputs(targets, queries):
    t_ids = np.unique(targets[1])
    q_indptr, q_indices, q_values = queries
    in_t = np.isin(q_indices, t_ids)
    assert 0 < in_t.sum() < in_t.size  # some query features occur in no target
    nq = q_indptr.size - 1
    live = np.array([np.any(q_values[q_indptr[r]:q_indptr[r + 1]] != 0) for r in range(nq)])
    alone = np.array([not in_t[q_indptr[r]:q_indptr[r + 1]].any() for r in range(nq)])
    assert (live & alone).any()  # non-zero queries that share no feature with any target
    assert (np.diff(q_indptr) == 0).any() and (~live & (np.diff(q_indptr) > 0)).any()  # empty and all-zero queries


@pytest.fixture(scope="module", params=METRICS)
def external(request, oracle):
    metric = request.param
    targets, queries, dup = _external(metric)
    _assert_external_inputs(targets, queries)
    ones = (queries[0], queries[1], None)
    if metric == "cosine":
        want = {(k, v): qmodel.cosine(oracle, targets, q, k)
                for k in (1, 20, 128) for v, q in (("values", queries), ("ones", ones))}
    else:
        dists = qmodel.jaccard_distances if metric == "jaccard" else qmodel.weighted_jaccard_distances
        args = (F,) if metric == "jaccard" else ()
        D = {"values": dists(targets, queries, *args), "ones": dists(targets, ones, *args)}
        want = {(k, v): qmodel.top_k_rows(D[v], k) for k in (1, 20, 128) for v in D}
    return metric, targets, queries, dup, want


@pytest.mark.parametrize("k", [1, 20, 128])
def test_external_queries_match_the_models(ctx, external, k):
    metric, targets, queries, dup, want = external
    nq = queries[0].size - 1
    with ctx.sparse_index(*targets, F, metric=metric) as index:
        got = index.query(*queries, k)
        t = ctx.last_knn_trace()
        blocks = index.query(*queries, k, block_rows=150)
        # queries without values (every stored entry 1) against the index built with values
        ones = index.query(queries[0], queries[1], None, k)
        t1 = ctx.last_knn_trace()
    _same(got, want[k, "values"])
    zero = int(_zero_rows(queries[0], queries[2], metric).sum())
    assert t["kind"] == "sparse" and t["queries"] == nq and t["targets"] == 3000 and t["k"] == k, t
    assert t["zero_queries"] == zero > 0, t
    assert k < 20 or 20 in got[0][dup]  # the copied target row is found (there is no self to leave out)
    _same(blocks, want[k, "values"])
    _same(ones, want[k, "ones"])
    assert t1["zero_queries"] == int((np.diff(queries[0]) == 0).sum()) < zero


def test_zero_queries_against_an_index_without_zero_rows(ctx, oracle):
    """The closed form of a zero query needs no zero row in the index: the first k rows at distance 1."""
    indptr, indices, values = _heavy_rows(200, seed=8)
    q = (np.array([0, 0, 2, 2], np.int64), np.array([0, 3], np.int32), np.array([0.0, -0.0], np.float32))
    for metric in METRICS:
        with ctx.sparse_index(indptr, indices, values, 1 << 24, metric=metric) as index:
            assert index.info()["zero_rows"] == 0
            idx, dist = index.query(*q, 7)
            assert ctx.last_knn_trace()["zero_queries"] == 3
        assert np.array_equal(idx, np.tile(np.arange(7, dtype=np.int32), (3, 1))) and np.all(dist == 1.0)


# ---- 4. external heavy queries ----------------------------------------------------------------------------------------
def test_external_heavy_queries_take_the_range_split(ctx, oracle):
    k, Fh = 20, 1 << 24
    targets = _heavy_rows(3000, seed=6)
    queries = _heavy_rows(300, seed=7)
    rows = np.unique(np.concatenate([[0, 299], np.random.default_rng(5).choice(np.arange(1, 299), 10, replace=False)]))
    with ctx.sparse_index(*targets, Fh) as index:
        got = index.query(*queries, k)
        t = ctx.last_knn_trace()
    assert t["queries"] == 300 and 0 < t["range_queries"] <= 300 and t["range_chunks"] == 6, t
    qmodel.check_cosine_rows(oracle, _row_norms, targets, queries, Fh, k, rows, got)
    with ctx.sparse_index(*targets, Fh, metric="jaccard") as index:
        got = index.query(*queries, k)
        assert ctx.last_knn_trace()["range_queries"] > 0
    sample = _cut(*queries, 0, 12)
    _same((got[0][:12], got[1][:12]), qmodel.top_k_rows(qmodel.jaccard_distances(targets, sample, Fh), k))


# ---- 5. edges ---------------------------------------------------------------------------------------------------------
def test_no_query_and_one_query(ctx, own):
    metric, indptr, indices, values = own
    with ctx.sparse_index(indptr, indices, values, F, metric=metric) as index:
        idx, dist = index.query(np.zeros(1, np.int64), np.zeros(0, np.int32), None, 20)
        assert idx.shape == dist.shape == (0, 20) and idx.dtype == np.int32 and dist.dtype == np.float32
        t = ctx.last_knn_trace()
        assert t["kind"] == "sparse" and t["queries"] == 0 and t["targets"] == 3001 and t["k"] == 20, t
        idx, dist = index.query(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 20, block_rows=3)
        assert idx.shape == (0, 20)
        _same(index.query(*_cut(indptr, indices, values, 1234, 1235), 20), index.search(20, 1234, 1235))
        assert ctx.last_knn_trace()["queries"] == 1


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 5, 64])
def test_k_equals_n_and_fewer_queries_than_k(ctx, oracle, n, metric):
    if metric == "weighted_jaccard":
        targets = weighted_rows(n, seed=n, F=1 << 24, n_ids=128, per=(1, 4))
    else:
        targets = _hard_rows(n, seed=n, F=1 << 24, n_ids=128, per=(1, 4))[:3]
    # four queries (fewer than k at n = 5 and 64, more at n = 1): over ids of the targets, empty, alone with an id of
    # its own, and a copy of the last target row
    first = np.unique(targets[1]).astype(np.int64)[:3]
    queries = rows_csr([(first, (0.37 * (1 + np.arange(first.size))).astype(np.float32)),
                        (np.zeros(0, np.int64), np.zeros(0, np.float32)),
                        (np.array([(1 << 24) - 1], np.int64), np.array([1.5], np.float32)),
                        _rows_of(*targets)[n - 1]])
    with ctx.sparse_index(*targets, 1 << 24, metric=metric) as index:
        _same(index.query(*targets, n), index.search(n))  # k == n, own rows
        got = index.query(*queries, n)
        assert got[0].shape == (4, n) and np.all(np.sort(got[0], axis=1) == np.arange(n))  # every row, once
    if metric == "cosine":
        want = qmodel.cosine(oracle, targets, queries, n)
    elif metric == "jaccard":
        want = qmodel.top_k_rows(qmodel.jaccard_distances(targets, queries, 1 << 24), n)
    else:
        want = qmodel.top_k_rows(qmodel.weighted_jaccard_distances(targets, queries), n)
    _same(got, want)


# ---- 6. refusals leave the index alone --------------------------------------------------------------------------------
def _raw_query(ctx, k, indptr, indices, values, results=True):
    nq = indptr.size - 1
    idx, dist = np.empty((nq, max(k, 1)), np.int32), np.empty((nq, max(k, 1)), np.float32)
    vp = ctypes.c_void_p
    rc = ctx._L.fdr_sparse_index_query(ctx._h, k, nq, vp(indptr.ctypes.data), vp(indices.ctypes.data),
                                       None if values is None else vp(values.ctypes.data),
                                       vp(idx.ctypes.data) if results else None,
                                       vp(dist.ctypes.data) if results else None)
    return rc, idx, dist


def _raw_search(ctx, k, lo, hi):
    idx, dist = np.empty((hi - lo, k), np.int32), np.empty((hi - lo, k), np.float32)
    vp = ctypes.c_void_p
    return ctx._L.fdr_sparse_index_search(ctx._h, k, lo, hi, vp(idx.ctypes.data), vp(dist.ctypes.data)), idx, dist


@pytest.mark.parametrize("metric", METRICS)
def test_a_refused_query_leaves_the_index_as_it_was(ctx, metric):
    Fs, n = 1 << 20, 200
    if metric == "weighted_jaccard":
        indptr, indices, values = weighted_rows(n, seed=2, F=Fs, n_ids=128)
    else:
        indptr, indices, values, _ = _hard_rows(n, seed=2, F=Fs, n_ids=128)
    code = _lib.SPARSE_METRICS[metric]
    vp = ctypes.c_void_p
    assert ctx._L.fdr_sparse_index_build(ctx._h, code, n, Fs, vp(indptr.ctypes.data), vp(indices.ctypes.data),
                                         vp(values.ctypes.data)) == 0
    rc, idx0, dist0 = _raw_search(ctx, 5, 0, n)
    assert rc == 0
    two = np.flatnonzero(np.diff(indptr) >= 2)[0]
    a = int(indptr[two])
    big = indices.copy()
    big[indptr[two + 1] - 1] = Fs  # an id >= F
    desc = indices.copy()
    desc[a], desc[a + 1] = indices[a + 1], indices[a]  # descending ids
    nan = values.copy()
    nan[a] = np.nan
    neg = np.abs(values)
    neg[a] = -0.37
    refused = [("range", 5, indptr, big, values, True), ("order", 5, indptr, desc, values, True),
               ("nan", 5, indptr, indices, nan, True), ("k = 0", 0, indptr, indices, values, True),
               ("k = n + 1", n + 1, indptr, indices, values, True), ("null results", 5, indptr, indices, values, False),
               ("indptr[0]", 5, indptr + 1, indices, values, True),
               ("monotone", 5, np.array([0, 3, 2], np.int64), indices, values, True)]
    if metric == "weighted_jaccard":
        refused.append(("negative", 5, indptr, indices, neg, True))
    for what, k, ip, ix, v, results in refused:
        assert _raw_query(ctx, k, ip, ix, v, results)[0] == E_ARG, what
        assert ctx._L.fdr_last_error(), what
        rc, idx, dist = _raw_search(ctx, 5, 0, n)
        assert rc == 0, what
        _same((idx, dist), (idx0, dist0))
    if metric != "weighted_jaccard":  # (a negative value is a value like any other under the other two metrics)
        assert _raw_query(ctx, 5, indptr, indices, neg)[0] == 0
    assert ctx._L.fdr_sparse_index_query(ctx._h, 5, -1, vp(indptr.ctypes.data), None, None, None, None) == E_ARG
    assert ctx._L.fdr_sparse_index_query(ctx._h, 5, 0, None, None, None, None, None) == 0  # nq = 0 needs no pointer
    rc, idx, dist = _raw_query(ctx, 5, indptr, indices, values)
    assert rc == 0
    _same((idx, dist), (idx0, dist0))
    assert ctx._L.fdr_sparse_index_free(ctx._h) == 0
    assert _raw_query(ctx, 5, indptr, indices, values)[0] == E_STATE
    assert b"no sparse index" in ctx._L.fdr_last_error()


# ---- 7. the index survives --------------------------------------------------------------------------------------------
def test_the_index_survives_queries_and_other_calls(ctx, external):
    metric, targets, queries, dup, want = external
    with ctx.sparse_index(*targets, F, metric=metric) as index:
        before = index.info()
        s20 = index.search(20)
        q20 = index.query(*queries, 20)
        mid = index.info()
        assert mid["device_bytes"] >= before["device_bytes"]
        assert {k: v for k, v in mid.items() if k != "device_bytes"} == \
            {k: v for k, v in before.items() if k != "device_bytes"}
        E = np.random.default_rng(12).standard_normal((700, 64)).astype(np.float32)
        E[::9] = 0.0
        ctx.knn(E, 10)
        assert ctx.last_knn_trace()["kind"] != "sparse"
        _same(index.search(20), s20)
        _same(index.query(*queries, 20), q20)
        assert index.info()["device_bytes"] >= mid["device_bytes"]
    _same(q20, want[20, "values"])


def test_query_raises_after_close(ctx):
    indptr, indices, values, _ = _hard_rows(64, seed=3, F=1 << 24, n_ids=128, per=(1, 4))
    index = ctx.sparse_index(indptr, indices, values, 1 << 24)
    index.query(indptr, indices, values, 5)
    index.close()
    with pytest.raises(_lib.FedrannHipError, match="closed"):
        index.query(indptr, indices, values, 5)


# ---- 8. target shards compose -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_target_shards_merge_into_the_whole_call(ctx, monkeypatch, metric):
    indptr, indices, values, Fs = _synth_idf(3000)
    n, k, world = indptr.size - 1, 20, 3
    built = []
    build = ctx.sparse_index

    def hook(*a, **kw):
        index = build(*a, **kw)
        built.append(index.info()["n"])
        return index

    monkeypatch.setattr(ctx, "sparse_index", hook)
    parts, covered = [], 0
    for rank in range(world):
        lo, hi, idx, dist = distributed.sparse_knn_target_shard(ctx, indptr, indices, values, Fs, k, rank, world,
                                                                metric=metric, block_rows=1100)
        assert lo == covered and idx.shape == dist.shape == (n, k)
        assert np.all((idx >= lo) & (idx < hi))
        covered = hi
        parts.append((idx, dist))
    assert covered == n and built == [hi - lo for lo, hi in distributed.shard_rows(n, world)[1]]
    assert all(abs(b - n / 3) < 0.05 * n for b in built), built
    monkeypatch.undo()
    want = ctx.knn_sparse(indptr, indices, values, Fs, k, metric=metric)
    _same(distributed.merge_sparse_topk(parts, k), want)
    _same(distributed.merge_sparse_topk(parts[::-1], k), want)
