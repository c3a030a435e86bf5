"""fdr_rescore_rows_*: the re-score rows held on the device, rectangular lists (X2 on the held rows) and ragged rows
with a bound in the exact metric (X3), against the numpy models of the sparse searches (tests/_radius_model.py), against
the exact radius search and against fdr_sparse_rescore.  Every comparison is exact: equal indptr, equal indices, equal
distance bit patterns."""
import ctypes

import numpy as np
import pytest

import _radius_model as rmodel
import _rescore_rows as rr
from _rescore_rows import F, N, T, WHICH
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = _lib.FDR_E_ARG, _lib.FDR_E_STATE
vp = ctypes.c_void_p
SENTINEL = -7


@pytest.fixture(scope="module")
def csr():
    return rr.rows()


@pytest.fixture(scope="module")
def matrices(csr, oracle):
    return rr.matrices(csr, oracle)


@pytest.fixture(scope="module")
def edges():
    return rr.ragged(rr.edge_lists())


def _held(ctx, csr, matrices, which):
    metric, values, D = matrices[which]
    return ctx.rescore_rows(csr[0], csr[1], values, F, metric=metric), D


# ---- 1. against the exact search ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
def test_all_rows_as_candidates_give_the_exact_radius_search(ctx, csr, matrices, which):
    metric, values, D = matrices[which]
    r, a, b = rr.between(D, 0.3)
    assert (D == a).any() and (D == b).any() and a <= r < b
    rng = np.random.default_rng(21)
    ip, ix = rr.ragged([rng.permutation(N) for _ in range(N)])  # 3 batches per query, the last one partial
    with ctx.sparse_index(csr[0], csr[1], values, F, metric=metric) as index:
        exact = index.radius_search(float(r))
    with ctx.rescore_rows(csr[0], csr[1], values, F, metric=metric) as held:
        got = held.radius(ip, ix, float(r))
    assert 0 < got[0][-1] < N * N
    rmodel.same(got, exact)
    rmodel.same(got, rr.want(D, 0, ip, ix, r))


# ---- 2. batch and tile edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
def test_batch_and_tile_edges_match_the_model(ctx, csr, matrices, edges, which):
    held, D = _held(ctx, csr, matrices, which)
    ip, ix = edges
    with held:
        for r in (rr.between(D, 0.6)[0], np.float32(1.0)):
            got = held.radius(ip, ix, float(r))
            rmodel.same(got, rr.want(D, 0, ip, ix, r))
    assert 0 < rr.want(D, 0, ip, ix, rr.between(D, 0.6)[0])[0][-1] < ix.size


# ---- 3. bounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
def test_bounds(ctx, csr, matrices, edges, which):
    held, D = _held(ctx, csr, matrices, which)
    ip, ix = edges
    with held:
        # r = 1: every candidate, in the exact order
        all_ = held.radius(ip, ix, 1.0)
        assert np.array_equal(all_[0], ip)
        rmodel.same(all_, rr.want(D, 0, ip, ix, 1.0))
        # r = 0: duplicates, self and zero pairs only
        zero = held.radius(ip, ix, 0.0)
        rmodel.same(zero, rr.want(D, 0, ip, ix, 0.0))
        assert 0 < zero[0][-1] < ix.size and np.all(zero[2] == 0)
        # r = -0.0 is r = 0, also where the sign bit reaches the library (the Python check clears it)
        rmodel.same(held.radius(ip, ix, -0.0), zero)
        out = np.full(ip.size, SENTINEL, np.int64)
        rc = ctx._L.fdr_rescore_rows_radius(ctx._h, ctypes.c_float(-0.0), 0, N, vp(ip.ctypes.data), vp(ix.ctypes.data),
                                            vp(out.ctypes.data))
        assert rc == 0 and np.array_equal(out, zero[0]), ctx._L.fdr_last_error()
        row = zero[1][zero[0][45]:zero[0][46]]  # a zero query (with values): the zero rows of its list, itself among them
        assert 45 in row and (0 in row or which == "jaccard_sets") and np.all(D[45, row] == 0)
        # r exactly a distance that occurs among the candidates: the bound is closed
        d_all = all_[2]
        inner = np.unique(d_all[(d_all > 0) & (d_all < 1)])
        r = np.float32(inner[inner.size // 2])
        assert (D == r).any() and (d_all == r).any()
        at = held.radius(ip, ix, float(r))
        rmodel.same(at, rr.want(D, 0, ip, ix, r))
        assert (at[2] == r).sum() == (d_all == r).sum() > 0
        # the prefix property: the result at r is the entries <= r of the result at 1
        counts = np.diff(at[0])
        for q in range(N):
            lo = all_[0][q]
            assert np.array_equal(at[1][at[0][q]:at[0][q + 1]], all_[1][lo:lo + counts[q]])
            assert np.all(all_[2][lo + counts[q]:all_[0][q + 1]] > r)


# ---- 4. call shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
def test_call_shapes(ctx, csr, matrices, edges, which):
    held, D = _held(ctx, csr, matrices, which)
    ip, ix = edges
    r = float(rr.between(D, 0.6)[0])
    with held:
        whole = held.radius(ip, ix, r)
        # a middle block of queries
        q_lo, nq = 37, 120
        ipb = np.ascontiguousarray(ip[q_lo:q_lo + nq + 1] - ip[q_lo])
        ixb = np.ascontiguousarray(ix[ip[q_lo]:ip[q_lo + nq]])
        got = held.radius(ipb, ixb, r, q_lo=q_lo)
        lo, hi = whole[0][q_lo], whole[0][q_lo + nq]
        rmodel.same(got, (whole[0][q_lo:q_lo + nq + 1] - lo, whole[1][lo:hi], whole[2][lo:hi]))
        # no query; every row empty
        none = held.radius(np.zeros(1, np.int64), np.zeros(0, np.int32), r, q_lo=N)
        assert list(none[0]) == [0] and none[1].size == none[2].size == 0
        empty = held.radius(np.zeros(11, np.int64), np.zeros(0, np.int32), r, q_lo=5)
        assert np.array_equal(empty[0], np.zeros(11, np.int64)) and empty[1].size == empty[2].size == 0
        # pieces: the uncut result
        cap = int(np.diff(ip).max())
        assert ix.size > 3 * cap
        rmodel.same(held.radius(ip, ix, r, max_entries=cap), whole)
        # one query above max_entries: refused by name, before the library is called
        big = int(np.argmax(np.diff(ip) > cap - 1))
        with pytest.raises(ValueError, match="query %d alone" % (3 + big)):
            held.radius(ip[:-3], ix[:ip[-4]], r, q_lo=3, max_entries=cap - 1)


# ---- 5. knn on the held rows ----------------------------------------------------------------------------------------------
def _lists(k_in, seed):
    rng = np.random.default_rng(seed)
    cand = np.stack([rng.permutation(N)[:k_in] for _ in range(N)]).astype(np.int32)
    if k_in > len(rr.SPECIAL) + 1:
        cand[:, :len(rr.SPECIAL)] = np.arange(len(rr.SPECIAL))
        cand[:, len(rr.SPECIAL)] = np.arange(N)
    return np.ascontiguousarray(cand)


def _fetch(ctx, hits):
    idx = np.full(max(hits, 1), SENTINEL, np.int32)
    dist = np.full(max(hits, 1), SENTINEL, np.float32)
    rc = ctx._L.fdr_rescore_rows_radius_fetch(ctx._h, hits, vp(idx.ctypes.data), vp(dist.ctypes.data))
    return rc, idx, dist, ctx._L.fdr_last_error().decode()


@pytest.mark.parametrize("which", WHICH)
def test_knn_on_held_rows_is_sparse_rescore(ctx, csr, matrices, edges, which):
    metric, values, D = matrices[which]
    ip, ix = edges
    with ctx.rescore_rows(csr[0], csr[1], values, F, metric=metric) as held:
        ragged = held.radius(ip, ix, 1.0)
        for k_in, k in ((1, 1), (20, 7), (128, 128)):
            cand = _lists(k_in, 300 + k_in)
            want = ctx.sparse_rescore(csr[0], csr[1], values, F, cand, k=k, metric=metric)
            got = held.knn(cand, k=k)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        part = held.knn(np.ascontiguousarray(cand[30:90]), q_lo=30)
        assert np.array_equal(part[0], want[0][30:90]) and np.array_equal(part[1].view(np.uint32), want[1][30:90].view(np.uint32))
        # the held radius result is still there
        rc, idx, dist, msg = _fetch(ctx, int(ragged[0][-1]))
        assert rc == 0, msg
        assert np.array_equal(idx, ragged[1]) and np.array_equal(dist.view(np.uint32), ragged[2].view(np.uint32))


# ---- 6. refusals leave the outputs untouched ------------------------------------------------------------------------------
def _raw_radius(ctx, radius, q_lo, ip, ix):
    out = np.full(ip.size, SENTINEL, np.int64)
    rc = ctx._L.fdr_rescore_rows_radius(ctx._h, radius, q_lo, ip.size - 1, vp(ip.ctypes.data), vp(ix.ctypes.data),
                                        vp(out.ctypes.data))
    return rc, out, ctx._L.fdr_last_error().decode()


def _raw_build(ctx, metric, indptr, indices, values):
    return ctx._L.fdr_rescore_rows_build(ctx._h, _lib.SPARSE_METRICS[metric], indptr.size - 1, F, vp(indptr.ctypes.data),
                                         vp(indices.ctypes.data), vp(values.ctypes.data) if values is not None else None)


def _raw_knn(ctx, q_lo, cand, k_out):
    idx = np.full((cand.shape[0], k_out), SENTINEL, np.int32)
    dist = np.full((cand.shape[0], k_out), SENTINEL, np.float32)
    rc = ctx._L.fdr_rescore_rows_knn(ctx._h, q_lo, cand.shape[0], cand.shape[1], vp(cand.ctypes.data), k_out,
                                     vp(idx.ctypes.data), vp(dist.ctypes.data))
    return rc, idx, dist, ctx._L.fdr_last_error().decode()


def _info_rc(ctx):
    return ctx._L.fdr_rescore_rows_info(ctx._h, None, None, None, None)


def _no_result(ctx):
    rc, idx, dist, _ = _fetch(ctx, 0)
    return rc == E_STATE and np.all(idx == SENTINEL) and np.all(dist == SENTINEL)


def test_refusals_write_nothing(ctx, csr, matrices, edges):
    metric, values, D = matrices["weighted_jaccard"]
    indptr, indices, _ = csr
    ip, ix = edges
    L = ctx._L
    # ---- without a row set: every call but _free is a state error ----
    assert L.fdr_rescore_rows_free(ctx._h) == 0 and L.fdr_rescore_rows_free(ctx._h) == 0
    assert _info_rc(ctx) == E_STATE
    rc, out, msg = _raw_radius(ctx, 0.5, 0, ip, ix)
    assert rc == E_STATE and np.all(out == SENTINEL), msg
    rc, idx, dist, msg = _raw_knn(ctx, 0, _lists(20, 1), 5)
    assert rc == E_STATE and np.all(idx == SENTINEL) and np.all(dist == SENTINEL), msg
    assert _fetch(ctx, 0)[0] == E_STATE
    # ---- a build with a row error leaves no row set, also where one was held ----
    assert _raw_build(ctx, metric, indptr, indices, values) == 0 and _info_rc(ctx) == 0
    swapped = indices.copy()
    a = int(indptr[3])
    swapped[a], swapped[a + 1] = indices[a + 1], indices[a]
    assert _raw_build(ctx, metric, indptr, swapped, values) == E_ARG and b"ascending" in L.fdr_last_error()
    assert _info_rc(ctx) == E_STATE and _raw_radius(ctx, 0.5, 0, ip, ix)[0] == E_STATE
    neg = values.copy()
    neg[int(np.flatnonzero(values > 0)[0])] *= -1
    assert _raw_build(ctx, metric, indptr, indices, neg) == E_ARG and b"negative" in L.fdr_last_error()
    assert _raw_build(ctx, "cosine", indptr, indices, neg) == 0  # (cosine takes signs)
    assert _raw_build(ctx, metric, np.ascontiguousarray(indptr + 1), indices, values) == E_ARG
    assert L.fdr_rescore_rows_build(ctx._h, 3, N, F, vp(indptr.ctypes.data), vp(indices.ctypes.data), None) == E_ARG
    assert _info_rc(ctx) == E_STATE
    # ---- the radius call's refusals ----
    assert _raw_build(ctx, metric, indptr, indices, values) == 0
    r = float(rr.between(D, 0.6)[0])
    rc, out, msg = _raw_radius(ctx, r, 0, ip, ix)
    assert rc == 0 and out[0] == 0, msg
    good = rr.want(D, 0, ip, ix, r)
    assert np.array_equal(out, good[0])
    # candidates outside [0, n): the smallest (query, position in its row) is named, nothing is held
    bad = ix.copy()
    q5 = [q for q in range(N) if ip[q + 1] - ip[q] > 200][:2]
    bad[ip[q5[1]] + 3] = -1
    bad[ip[q5[0]] + 190] = N
    bad[ip[q5[0]] + 199] = -1
    rc, out, msg = _raw_radius(ctx, r, 0, ip, bad)
    assert rc == E_ARG and np.all(out == SENTINEL) and "query %d, position 190" % q5[0] in msg and "(%d)" % N in msg, msg
    assert _no_result(ctx)
    q_lo = 10
    ipb = np.ascontiguousarray(ip[q_lo:q_lo + 101] - ip[q_lo])
    ixb = np.ascontiguousarray(ix[ip[q_lo]:ip[q_lo + 100]])
    bad = ixb.copy()
    bad[-1] = -1
    last = int(np.flatnonzero(np.diff(ipb) > 0)[-1])
    rc, out, msg = _raw_radius(ctx, r, q_lo, ipb, bad)
    where = "query %d, position %d" % (q_lo + last, ipb[last + 1] - ipb[last] - 1)
    assert rc == E_ARG and np.all(out == SENTINEL) and where in msg and "(-1)" in msg, msg
    with pytest.raises(_lib.FedrannHipError, match="position"):
        _lib.RescoreRows(ctx, N, metric, ctx._rescore_gen).radius(ipb, bad, r, q_lo=q_lo)
    # the indptr rules, on the host
    off = ip.copy()
    off[0] = 1
    rc, out, msg = _raw_radius(ctx, r, 0, off, ix)
    assert rc == E_ARG and np.all(out == SENTINEL) and "starts at" in msg, msg
    down = ip.copy()
    down[7] = down[6] - 1
    rc, out, msg = _raw_radius(ctx, r, 0, down, ix)
    assert rc == E_ARG and np.all(out == SENTINEL) and "decreases" in msg, msg
    rc, out, msg = _raw_radius(ctx, r, N - 50, ipb, ixb)  # q_lo + nq > n
    assert rc == E_ARG and np.all(out == SENTINEL), msg
    assert _raw_radius(ctx, r, -1, ipb, ixb)[0] == E_ARG
    # the radius domain
    for radius in (float("nan"), -0.1, 1.5):
        rc, out, msg = _raw_radius(ctx, radius, 0, ip, ix)
        assert rc == E_ARG and np.all(out == SENTINEL) and "radius" in msg, (radius, msg)
        assert _no_result(ctx)
    # a fetch with the wrong number of hits
    rc, out, msg = _raw_radius(ctx, r, 0, ip, ix)
    assert rc == 0
    hits = int(out[-1])
    for wrong in (hits - 1, hits + 1, 0):
        rc, idx, dist, msg = _fetch(ctx, wrong)
        assert rc == E_ARG and np.all(idx == SENTINEL) and np.all(dist == SENTINEL), msg
    rc, idx, dist, msg = _fetch(ctx, hits)
    assert rc == 0 and np.array_equal(idx, good[1]) and np.array_equal(dist.view(np.uint32), good[2].view(np.uint32))
    # the rectangular call's refusals and limits are fdr_sparse_rescore's
    cand = _lists(20, 5)[10:110].copy()
    cand[5, 3] = N
    cand[9, 0] = -1
    rc, idx, dist, msg = _raw_knn(ctx, 10, cand, 9)
    assert rc == E_ARG and np.all(idx == SENTINEL) and np.all(dist == SENTINEL) and "query 15, slot 3" in msg, msg
    for k_in, k_out in ((20, 21), (20, 0), (129, 5)):
        rc, idx, dist, msg = _raw_knn(ctx, 10, np.zeros((100, k_in), np.int32), k_out)
        assert rc == E_ARG and np.all(idx == SENTINEL) and "k_" in msg, (k_in, k_out, msg)
    assert _fetch(ctx, hits)[0] == 0  # (and they leave the held result)
    assert L.fdr_rescore_rows_free(ctx._h) == 0 and _info_rc(ctx) == E_STATE


# ---- 7. independence ------------------------------------------------------------------------------------------------------
def test_the_row_set_and_the_indexes_do_not_touch_each_other(ctx, csr, matrices, edges):
    metric, values, D = matrices["weighted_jaccard"]
    indptr, indices, _ = csr
    ip, ix = edges
    rng = np.random.default_rng(3)
    r = float(rr.between(D, 0.6)[0])
    with ctx.sparse_index(indptr, indices, values, F, metric=metric) as sparse, \
            ctx.dense_index(rng.standard_normal((N, 64)).astype(np.float32)) as dense, \
            ctx.rescore_rows(indptr, indices, values, F, metric=metric) as held:
        knn_sparse = sparse.search(10)
        held_sparse = sparse.radius_search(r)
        held_dense = dense.radius_search(0.9)
        trace = ctx.last_knn_trace()
        ragged = held.radius(ip, ix, r)
        rmodel.same(ragged, rr.want(D, 0, ip, ix, r))
        bytes_before = held.info()["device_bytes"]
        assert held.info() == {"metric": metric, "n": N, "stored": int(indptr[-1]), "device_bytes": bytes_before}

        def fetch(symbol, total):
            idx, dist = np.empty(total, np.int32), np.empty(total, np.float32)
            assert getattr(ctx._L, symbol)(ctx._h, total, vp(idx.ctypes.data), vp(dist.ctypes.data)) == 0
            return idx, dist

        def all_held():
            for symbol, res in (("fdr_sparse_index_radius_fetch", held_sparse), ("fdr_dense_index_radius_fetch", held_dense),
                                ("fdr_rescore_rows_radius_fetch", ragged)):
                idx, dist = fetch(symbol, int(res[0][-1]))
                assert np.array_equal(idx, res[1]) and np.array_equal(dist.view(np.uint32), res[2].view(np.uint32)), symbol

        all_held()
        # fdr_sparse_rescore and the rectangular call on the held rows, in between
        cand = _lists(20, 5)
        a = ctx.sparse_rescore(indptr, indices, values, F, cand, k=9, metric=metric)
        b = held.knn(cand, k=9)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        all_held()
        assert ctx.last_knn_trace() == trace
        # the indexes' own calls leave the row set's result; the row set's leave theirs
        again = sparse.search(10)
        assert np.array_equal(again[0], knn_sparse[0]) and np.array_equal(again[1].view(np.uint32), knn_sparse[1].view(np.uint32))
        rmodel.same(dense.radius_search(0.9), held_dense)
        rmodel.same(sparse.radius_search(r), held_sparse)
        idx, dist = fetch("fdr_rescore_rows_radius_fetch", int(ragged[0][-1]))
        assert np.array_equal(idx, ragged[1]) and np.array_equal(dist.view(np.uint32), ragged[2].view(np.uint32))
        small = held.radius(ip[:5].copy(), ix[:ip[4]].copy(), 1.0)
        assert np.array_equal(small[0], ip[:5])
        for symbol, res in (("fdr_sparse_index_radius_fetch", held_sparse), ("fdr_dense_index_radius_fetch", held_dense)):
            idx, dist = fetch(symbol, int(res[0][-1]))
            assert np.array_equal(idx, res[1]) and np.array_equal(dist.view(np.uint32), res[2].view(np.uint32)), symbol
        rmodel.same(held.radius(ip, ix, r), ragged)
        assert held.info()["device_bytes"] >= bytes_before
    # a row set of the replaced generation raises
    with ctx.rescore_rows(indptr, indices, values, F, metric=metric) as first:
        weighted_bytes = first.info()["device_bytes"]
        with ctx.rescore_rows(indptr, indices, None, F, metric="jaccard") as second:
            # (a build under another metric releases what it does not use: 4 bytes per stored entry here)
            assert second.info()["device_bytes"] <= weighted_bytes - 4 * int(indptr[-1]) + 4 * N
            with pytest.raises(_lib.FedrannHipError, match="another"):
                first.radius(ip, ix, r)
            assert second.info()["metric"] == "jaccard"
