"""fdr_sparse_rescore: candidate lists re-scored by exact distance on the sparse rows, against the numpy models of the
sparse searches (tests/_radius_model.py, tests/_sparse_query_model.py) and against the search itself.  The expected row
of a query is D[q, candidates] of the model's full distance matrix, sorted by (distance bits, index), its first k_out.
Every comparison is exact: equal indices, equal distance bit patterns."""
import ctypes

import numpy as np
import pytest

import _radius_model as rmodel
from _weighted_rows import csr as rows_csr
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

E_ARG = -1
F = 1 << 20
N = 300
T = _lib.FDR_RESCORE_TILE
METRICS = ("cosine", "jaccard", "weighted_jaccard")
SPECIAL = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)  # row i of the fixture has SPECIAL[i] stored entries
N_ISO = 6  # rows whose ids no other row holds: their k-NN lists are themselves and the distance-1 fill
vp = ctypes.c_void_p


def _rows(seed=11):
    """N rows over ids spread across [0, F): the SPECIAL lengths first (the long ones drawn from the whole pool, so they
    share about half their ids with each other and cross the tile edges as query and as candidate), then short rows from
    a small sub-pool (so that most pairs share something), with stored zeros, duplicates, zero rows and isolated rows.
    Values on a coarse grid: equal distances occur."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(F, 2 * T + 1024 + N_ISO, replace=False)).astype(np.int64)
    iso, pool = pool[-N_ISO:], pool[:-N_ISO]
    rows = []
    for i in range(N):
        m = SPECIAL[i] if i < len(SPECIAL) else int(rng.integers(1, 41))
        ids = np.sort(rng.choice(pool if m > 40 else pool[:256], m, replace=False))
        vals = (rng.integers(1, 6, size=m) * 0.37).astype(np.float32)
        vals[rng.random(m) < 0.1] = 0.0  # explicit stored zeros
        rows.append((ids, vals))
    for i in (40, 140):
        rows[i] = (np.zeros(0, np.int64), np.zeros(0, np.float32))  # empty rows
    for i in (45, 145):
        ids = rows[i][0]
        rows[i] = (ids, np.where(np.arange(ids.size) % 2 == 0, 0.0, -0.0).astype(np.float32))  # only +-0: zero rows
    for i in (50, 150, 250):
        rows[i] = rows[20]  # duplicates
    rows[60] = rows[len(SPECIAL) - 1]  # a duplicate of the longest row
    for j in range(N_ISO):
        rows[70 + 10 * j] = (iso[j:j + 1], np.array([1.5], np.float32))
    return rows_csr(rows)


def _values(metric, values, seed=12):
    """cosine takes signs too; the Jaccard metrics the values as they are"""
    if metric != "cosine":
        return values
    sign = np.where(np.random.default_rng(seed).random(values.size) < 0.3, -1.0, 1.0).astype(np.float32)
    return values * sign


def _matrix(metric, oracle, csr, n_features):
    """float32 [n, n]: every row against every row under the models of the searches"""
    if metric == "cosine":
        idx, dist = rmodel.cosine_ranked(oracle, csr, csr)
        D = np.empty(idx.shape, np.float32)
        np.put_along_axis(D, idx.astype(np.int64), dist, axis=1)
        return D
    return rmodel.distances(metric, csr, csr, n_features)


def _want(D, q_lo, cand, k_out):
    idx = np.empty((cand.shape[0], k_out), np.int32)
    dist = np.empty((cand.shape[0], k_out), np.float32)
    for r in range(cand.shape[0]):
        d = D[q_lo + r, cand[r]]
        order = np.lexsort((cand[r], d.view(np.uint32)))[:k_out]  # (last key first: distance bits, then index)
        idx[r], dist[r] = cand[r][order], d[order]
    return idx, dist


def _same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1) | (got[1].view(np.uint32) != want[1].view(np.uint32)).any(axis=1))
    assert bad.size == 0, "rows %s differ; first: got %s %s, want %s %s" % (
        bad[:8], got[0][bad[0]], got[1][bad[0]], want[0][bad[0]], want[1][bad[0]])


def _candidates(k_in, seed):
    """[N, k_in]: distinct random rows, then the special rows and the query itself written over some slots (so a list
    may hold an index twice: it comes out twice)"""
    rng = np.random.default_rng(seed)
    cand = np.stack([rng.permutation(N)[:k_in] for _ in range(N)]).astype(np.int32)
    if k_in == 1:
        cand[:, 0] = (np.arange(N) * 7 + 3) % N
        cand[::3, 0] = np.arange(N)[::3] % len(SPECIAL)  # every third query meets a special row
        cand[::10, 0] = np.arange(N)[::10]  # ... every tenth itself
        return cand
    cand[:, :len(SPECIAL)] = np.arange(len(SPECIAL))
    cand[:, len(SPECIAL)] = np.arange(N)
    cand[:, len(SPECIAL) + 1] = 60  # the longest row's duplicate
    return np.ascontiguousarray(cand[:, rng.permutation(k_in)])


@pytest.fixture(scope="module")
def rows():
    return _rows()


@pytest.fixture(scope="module")
def matrices(rows, oracle):
    """metric -> (values, D); "jaccard_sets": Jaccard without values (every stored entry present)"""
    indptr, indices, values = rows
    out = {}
    for metric in METRICS:
        v = _values(metric, values)
        out[metric] = (v, _matrix(metric, oracle, (indptr, indices, v), F))
    out["jaccard_sets"] = (None, _matrix("jaccard", oracle, (indptr, indices, None), F))
    return out


# ---- 1. lane and tile edges -------------------------------------------------------------------------------------------
def test_the_fixture_has_the_edges(rows):
    indptr, indices, values = rows
    lens = np.diff(indptr)
    assert tuple(lens[:len(SPECIAL)]) == SPECIAL and lens[60] == 2 * T + 3
    assert lens[40] == 0 and np.all(values[indptr[45]:indptr[46]] == 0) and lens[45] > 0


@pytest.mark.parametrize("k_in, k_out", [(1, 1), (20, 20), (20, 7), (128, 128), (128, 50)])
@pytest.mark.parametrize("which", METRICS + ("jaccard_sets",))
def test_lane_and_tile_edges_match_the_model(ctx, rows, matrices, which, k_in, k_out):
    indptr, indices, _ = rows
    metric = "jaccard" if which == "jaccard_sets" else which
    values, D = matrices[which]
    cand = _candidates(k_in, seed=100 + k_in)
    got = ctx.sparse_rescore(indptr, indices, values, F, cand, k=k_out, metric=metric)
    assert got[0].shape == got[1].shape == (N, k_out)
    _same(got, _want(D, 0, cand, k_out))
    if k_in == k_out:  # k=None: every candidate comes back
        _same(ctx.sparse_rescore(indptr, indices, values, F, cand, metric=metric), got)
    if k_in > 1:  # the query's own index is an ordinary candidate, at its distance (0, or cosine's rounding of it)
        q = len(SPECIAL) + 3
        j = list(got[0][q]).index(q)
        assert got[1][q, j] == D[q, q] <= 2e-6


# ---- 2. closed forms and ties -----------------------------------------------------------------------------------------
def _small(metric):
    a_ids, a_vals = np.array([5, 9, 100]), np.array([1.0, 2.0, 3.0], np.float32)
    rows = [
        (np.zeros(0, np.int64), np.zeros(0, np.float32)),             # 0 empty
        (np.array([5, 9]), np.array([0.0, -0.0], np.float32)),        # 1 stored +-0 only: a zero row under every metric
        (a_ids, a_vals),                                              # 2 A
        (a_ids, a_vals),                                              # 3 A again
        (a_ids, a_vals),                                              # 4 and again
        (np.array([7, 11]), np.array([1.0, 4.0], np.float32)),        # 5 shares nothing with A
        (np.array([5, 9, 200]), np.array([-0.0, 2.0, 1.0], np.float32)),  # 6 holds 5 with a stored zero: absent
        (a_ids, -a_vals if metric != "weighted_jaccard" else 2 * a_vals),  # 7 -A: similarity -1 (weighted: 2 A)
        (np.zeros(0, np.int64), np.zeros(0, np.float32)),             # 8 empty
        (np.array([5, 300]), np.array([2.0, 0.0], np.float32)),       # 9 shares 5 with A; 300 stored as zero
    ]
    return rows_csr(rows)


@pytest.mark.parametrize("metric", METRICS)
def test_closed_forms_and_ties(ctx, oracle, metric):
    indptr, indices, values = _small(metric)
    n = indptr.size - 1
    D = _matrix(metric, oracle, (indptr, indices, values), 512)
    cand = np.ascontiguousarray(np.tile(np.arange(n - 1, -1, -1, dtype=np.int32), (n, 1)))  # every row, descending
    got = ctx.sparse_rescore(indptr, indices, values, 512, cand, metric=metric)
    _same(got, _want(D, 0, cand, n))
    one, zero = np.float32(1).view(np.uint32), np.uint32(0)
    bits = got[1].view(np.uint32)
    for q in (0, 1, 8):  # a zero query: the zero rows at 0 in index order, every other row at exactly 1
        assert list(got[0][q]) == [0, 1, 8, 2, 3, 4, 5, 6, 7, 9]
        assert np.all(bits[q, :3] == zero) and np.all(bits[q, 3:] == one)
    # A: itself and its duplicates at one distance (0; cosine: 1 - the rounded chain) in index order; a zero row and a
    # row that shares nothing at exactly 1
    assert list(got[0][2][:3]) == [2, 3, 4] and np.all(bits[2, :3] == bits[2, 0]) and got[1][2, 0] <= 2e-7
    assert metric == "cosine" or bits[2, 0] == zero
    at = {int(t): bits[2, j] for j, t in enumerate(got[0][2])}
    assert at[0] == at[1] == at[8] == at[5] == one
    assert zero < at[6] < one and zero < at[9] < one
    if metric == "cosine":
        assert at[7] == one  # similarity -1: clamped
    if metric == "jaccard":
        assert got[1][2][list(got[0][2]).index(6)] == np.float32((4 - 1) / 4)  # the stored zero of row 6 is absent
        assert got[1][2][list(got[0][2]).index(7)] == 0  # signs do not matter to a set
    if metric == "weighted_jaccard":
        assert got[1][2][list(got[0][2]).index(7)] == np.float32(0.5)  # sum of minima 6, of maxima 12
    assert np.all(got[1][:, 0] == np.diag(D)) and np.all(np.diag(D) <= 2e-7)  # every row finds itself first


# ---- 3. the window ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_a_window_gives_the_rows_of_the_whole_call(ctx, rows, matrices, metric):
    indptr, indices, _ = rows
    values = matrices[metric][0]
    cand = _candidates(20, seed=5)
    whole = ctx.sparse_rescore(indptr, indices, values, F, cand, k=9, metric=metric)
    for q_lo, nq in ((37, 100), (0, 10), (N - 1, 1)):
        part = np.ascontiguousarray(cand[q_lo:q_lo + nq])
        got = ctx.sparse_rescore(indptr, indices, values, F, part, k=9, metric=metric, q_lo=q_lo)
        _same(got, (whole[0][q_lo:q_lo + nq], whole[1][q_lo:q_lo + nq]))
    out = (np.full((0, 9), -7, np.int32), np.full((0, 9), -7, np.float32))
    got = ctx.sparse_rescore(indptr, indices, values, F, np.zeros((0, 20), np.int32), k=9, metric=metric, q_lo=N, out=out)
    assert got[0] is out[0] and got[0].shape == (0, 9)  # nq == 0: nothing to do


# ---- 4. fixed point against the search --------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_the_lists_of_the_search_come_back_unchanged(ctx, rows, matrices, metric):
    indptr, indices, _ = rows
    values = matrices[metric][0]
    k = 20
    idx, dist = ctx.knn_sparse(indptr, indices, values, F, k, metric=metric)
    assert dist[70, 0] == 0 and np.all(dist[70, 1:] == 1)  # an isolated row: itself, then the distance-1 fill
    nz = sum(1 for r in range(N) if not np.any(values[indptr[r]:indptr[r + 1]] != 0))  # zero rows (the empty ones too)
    assert 5 <= nz < k and np.all(dist[40, :nz] == 0) and np.all(dist[40, nz:] == 1)  # a zero query's closed-form row
    got = ctx.sparse_rescore(indptr, indices, values, F, idx, metric=metric)
    _same(got, (idx, dist))


# ---- 5. refusals leave the outputs untouched; the indexes and the trace stay ------------------------------------------
def _raw(ctx, metric, indptr, indices, values, n_features, q_lo, cand, k_out):
    nq, k_in = cand.shape
    idx = np.full((nq, k_out), -7, np.int32)
    dist = np.full((nq, k_out), -7, np.float32)
    rc = ctx._L.fdr_sparse_rescore(ctx._h, _lib.SPARSE_METRICS[metric], indptr.size - 1, n_features, vp(indptr.ctypes.data),
                                   vp(indices.ctypes.data), vp(values.ctypes.data) if values is not None else None, q_lo,
                                   nq, k_in, vp(cand.ctypes.data), k_out, vp(idx.ctypes.data), vp(dist.ctypes.data))
    return rc, idx, dist, ctx._L.fdr_last_error().decode()


def _untouched(idx, dist):
    return bool(np.all(idx == -7) and np.all(dist == -7))


def test_refusals_write_nothing_and_touch_neither_index_nor_trace(ctx, rows, matrices):
    indptr, indices, _ = rows
    values = matrices["weighted_jaccard"][0]
    rng = np.random.default_rng(3)
    with ctx.sparse_index(indptr, indices, values, F, metric="weighted_jaccard") as sparse, \
            ctx.dense_index(rng.standard_normal((N, 64)).astype(np.float32)) as dense:
        held_dense = dense.radius_search(0.9)
        held_sparse = sparse.search(10)
        trace = ctx.last_knn_trace()
        cand = np.ascontiguousarray(_candidates(20, seed=5)[10:110])
        # a fine call
        rc, idx, dist, _ = _raw(ctx, "weighted_jaccard", indptr, indices, values, F, 10, cand, 9)
        assert rc == 0
        _same((idx, dist), _want(matrices["weighted_jaccard"][1], 10, cand, 9))
        # candidates outside [0, n): the smallest (query, slot) is named
        bad = cand.copy()
        bad[9, 0] = -1
        bad[5, 3] = N
        bad[5, 17] = -1
        rc, idx, dist, msg = _raw(ctx, "weighted_jaccard", indptr, indices, values, F, 10, bad, 9)
        assert rc == E_ARG and _untouched(idx, dist) and "query 15, slot 3" in msg and "(%d)" % N in msg, msg
        bad = cand.copy()
        bad[99, 19] = -1
        rc, idx, dist, msg = _raw(ctx, "cosine", indptr, indices, values, F, 10, bad, 20)
        assert rc == E_ARG and _untouched(idx, dist) and "query 109, slot 19" in msg and "(-1)" in msg, msg
        with pytest.raises(_lib.FedrannHipError, match="slot 19"):
            ctx.sparse_rescore(indptr, indices, values, F, bad, metric="jaccard", q_lo=10)
        # the rows' own violations, found on the device
        neg = values.copy()
        neg[int(np.flatnonzero(values > 0)[0])] *= -1
        rc, idx, dist, msg = _raw(ctx, "weighted_jaccard", indptr, indices, neg, F, 10, cand, 9)
        assert rc == E_ARG and _untouched(idx, dist) and "negative" in msg, msg
        assert _raw(ctx, "cosine", indptr, indices, neg, F, 10, cand, 9)[0] == 0  # (cosine takes signs)
        swapped = indices.copy()
        a = int(indptr[3])
        swapped[a], swapped[a + 1] = indices[a + 1], indices[a]
        for metric in METRICS:
            rc, idx, dist, msg = _raw(ctx, metric, indptr, swapped, values, F, 10, cand, 9)
            assert rc == E_ARG and _untouched(idx, dist) and "ascending" in msg, (metric, msg)
        # the limits
        for k_in, k_out in ((20, 21), (20, 0), (129, 5)):
            rc, idx, dist, msg = _raw(ctx, "cosine", indptr, indices, values, F, 10, np.zeros((100, k_in), np.int32), k_out)
            assert rc == E_ARG and _untouched(idx, dist) and "k_" in msg, (k_in, k_out, msg)
        assert _raw(ctx, "cosine", indptr, indices, values, F, N - 50, cand, 9)[0] == E_ARG  # q_lo + nq > n
        assert _raw(ctx, "cosine", indptr, indices, values, F, -1, cand, 9)[0] == E_ARG
        rc = ctx._L.fdr_sparse_rescore(ctx._h, 3, N, F, vp(indptr.ctypes.data), vp(indices.ctypes.data), None, 10, 100, 20,
                                       vp(cand.ctypes.data), 9, vp(idx.ctypes.data), vp(dist.ctypes.data))
        assert rc == E_ARG and b"metric" in ctx._L.fdr_last_error()
        # neither index nor the trace has been touched
        assert ctx.last_knn_trace() == trace
        again = sparse.search(10)
        assert np.array_equal(again[0], held_sparse[0]) and \
            np.array_equal(again[1].view(np.uint32), held_sparse[1].view(np.uint32))
        rmodel.same(dense.radius_search(0.9), held_dense)
