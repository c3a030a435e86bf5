"""Radius search on the dense index (fdr_dense_index_build / _embed / _radius_search / _radius_query / _radius_fetch /
_info / _free) against the oracle (tests/_dense_radius_model.py: the oracle's ranking of ALL rows, cut at r).  Every
comparison is exact: equal indptr, equal indices, equal distance bit patterns.  The radii come from the oracle's own
distances; on the adversarial sets they include a boundary where a hit's fp16 distance lies above r, so a range pass
without the margin fails here (tests/test_dense_radius_host.py shows that on the CPU)."""
import ctypes

import numpy as np
import pytest

import _dense_radius_model as dmodel
import _dense_rows
import _radius_model as rmodel
from conftest import golden_embed_case
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5
ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))
vp = ctypes.c_void_p
# The planner never cuts a segment shorter than 4096 rows, so 4097 rows are the fewest that give two (2500: one); from
# 4096 queries a call runs on the ping-pong kernels, below on the four-wave ones.
N_TWO_SEGMENTS = 4097


def plain_rows(n, d, seed):
    """Rows around a few centres, with exact duplicates and (from 31 rows) zero rows."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((max(1, n // 8), d))
    E = (base[rng.integers(0, base.shape[0], size=n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    if n >= 31:
        E[rng.choice(n, size=4, replace=False)] = E[rng.choice(n, size=4, replace=False)]
        E[[3, n // 2, n - 1]] = 0.0
    return np.ascontiguousarray(E)


def _row(res, i):
    return res[1][res[0][i]:res[0][i + 1]], res[2][res[0][i]:res[0][i + 1]]


def _slice(res, a, b):
    ip = res[0]
    return ip[a:b + 1] - ip[a], res[1][ip[a]:ip[b]], res[2][ip[a]:ip[b]]


# ---- 1. parity with the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 100, 256, 500])
@pytest.mark.parametrize("n", [1, 31, 33, 1000, 2500])
def test_shapes_match_the_model(ctx, oracle, n, d):
    E = plain_rows(n, d, 31 * n + d)
    want = dmodel.model(oracle, E)
    D, Dt = dmodel.exact_dists(oracle, E), dmodel.approx_dists(oracle, E)
    radii = dmodel.radii(D, Dt) if n > 1 else [np.float32(0.0), np.float32(0.5)]
    if n <= 33:
        radii.append(ONE_BELOW)  # (every row is a candidate)
    with ctx.dense_index(E) as index:
        for r in radii:
            got = index.radius_search(r)
            info = index.info()
            print("n = %d d = %d r = %.9g: %d hits of %d candidates, %d x %d work items"
                  % (n, d, r, got[0][-1], info["last_candidates"], info["last_query_blocks"], info["last_segments"]))
            rmodel.same(got, want(r))
            assert info["last_hits"] == got[0][-1] <= info["last_candidates"]
            assert info["n"] == n and info["d"] == d and info["device_bytes"] > 0
        if n == 2500:
            assert info["last_query_blocks"] >= 2
        if n == 1:
            assert got[0][-1] == 1 and got[1][0] == 0  # self


@pytest.fixture(scope="module", params=["%s-%d" % s for s in dmodel.ADVERSARIAL] + ["mixed-100"])
def hard_set(request, oracle):
    name = request.param
    kind, d = name.rsplit("-", 1)
    E = dmodel.mixed() if kind == "mixed" else dmodel.adversarial(kind, int(d))
    D, Dt = dmodel.exact_dists(oracle, E), dmodel.approx_dists(oracle, E)
    return name, E, dmodel.model(oracle, E), dmodel.radii(D, Dt), D, Dt, dmodel.scanned(oracle, E)


def test_adversarial_sets_match_the_model(ctx, hard_set):
    name, E, want, radii, D, Dt, live = hard_set
    with ctx.dense_index(E) as index:
        for r in radii:
            got = index.radius_search(r)
            above = int(((D <= r) & (Dt > r) & live[:, None]).sum())
            print("%s r = %.9g: %d hits (%d with an fp16 distance above r), %d candidates"
                  % (name, r, got[0][-1], above, index.info()["last_candidates"]))
            rmodel.same(got, want(r))


def test_a_radius_inside_a_plateau(ctx, oracle):
    E = _dense_rows.clusters(600, 100, 5)
    idx, dist = dmodel.ranked(oracle, E)
    q = 200
    r = dist[q, 80]  # the 80th neighbour of a cluster member: inside its cluster's plateau of near ties
    assert dist[q, 60] < 1 and dist[q, 100] < 1 and dist[q, 100] - dist[q, 60] < 1e-4
    want = rmodel.cut_ranked(idx, dist, r)
    with ctx.dense_index(E) as index:
        got = index.radius_search(r)
    rmodel.same(got, want)
    assert np.diff(got[0]).max() > 80


# ---- 2. row ranges, blocks and segments --------------------------------------------------------------------------------
_TWO_SEGMENTS = {}


def _two_segments(oracle, d):
    if d not in _TWO_SEGMENTS:
        E = plain_rows(N_TWO_SEGMENTS, d, 77 + d)
        idx, dist = dmodel.ranked(oracle, E)
        r = np.sort(dist[:, 6])[N_TWO_SEGMENTS // 2]  # about six hits a row
        _TWO_SEGMENTS[d] = (E, r, rmodel.cut_ranked(idx, dist, r))
    return _TWO_SEGMENTS[d]


@pytest.fixture(scope="module", params=[8, 256, 500])  # (dp = 128, 256, 512: every ping-pong and four-wave instance)
def two_segments(request, oracle):
    return _two_segments(oracle, request.param)


def test_two_segments_and_row_ranges(ctx, two_segments):
    E, r, want = two_segments
    n = E.shape[0]
    with ctx.dense_index(E) as index:
        got = index.radius_search(r)  # 4097 queries: the ping-pong kernels
        info = index.info()
        print(info)
        rmodel.same(got, want)
        assert info["last_query_blocks"] >= 2 and info["last_segments"] >= 2
        # lo not a multiple of 32; across a query-block boundary (128 queries); shorter than a tile; to the last row
        for lo, hi in ((5, 37), (100, 300), (1000, 1007), (4000, n), (1, 2500)):
            part = index.radius_search(r, lo, hi)  # fewer than 4096 queries: the four-wave kernels
            info = index.info()
            rmodel.same(part, _slice(want, lo, hi))
            assert info["last_segments"] >= 2 and info["last_hits"] == part[0][-1]
        empty = index.radius_search(r, 17, 17)
        assert empty[0].tolist() == [0] and empty[1].size == 0 and empty[2].size == 0
        # the rows as outside queries: the same bits; in blocks too
        for lo, hi in ((5, 37), (1000, 1300)):
            rmodel.same(index.radius_query(E[lo:hi], r), _slice(want, lo, hi))
        rmodel.same(index.radius_query(E[64:400], r, block_rows=100), _slice(want, 64, 400))
        none = index.radius_query(np.zeros((0, E.shape[1]), np.float32), r)
        assert none[0].tolist() == [0] and none[1].size == 0


# ---- 3. zero rows ------------------------------------------------------------------------------------------------------
def test_zero_queries_and_zero_targets(ctx, oracle):
    E = plain_rows(300, 100, 9)
    zero = np.flatnonzero(~E.any(axis=1))
    assert zero.tolist() == [3, 150, 299]
    with ctx.dense_index(E) as index:
        for r in (np.float32(0.0), np.float32(0.3), ONE_BELOW):
            got = index.radius_search(r)
            rmodel.same(got, dmodel.model(oracle, E)(r))
            for q in zero:  # all zero rows, index order, distance 0
                ix, ds = _row(got, q)
                assert ix.tolist() == zero.tolist() and not ds.any()
            hit_by_others = np.setdiff1d(np.arange(300), zero)
            for q in hit_by_others[:50]:  # a non-zero query never hits a zero row
                assert not np.isin(_row(got, q)[0], zero).any()
        Q = np.concatenate([np.zeros((2, 100), np.float32), E[10:12]])
        got = index.radius_query(Q, 0.3)
        rmodel.same(got, dmodel.model(oracle, E, Q)(np.float32(0.3)))
        assert _row(got, 0)[0].tolist() == zero.tolist()
    nz = E[E.any(axis=1)]
    with ctx.dense_index(nz) as index:  # a set without zero rows: a zero query finds nothing
        got = index.radius_query(np.zeros((3, 100), np.float32), 0.5)
        assert got[0].tolist() == [0, 0, 0, 0]
        rmodel.same(index.radius_search(0.2), dmodel.model(oracle, nz)(np.float32(0.2)))


# ---- 4. consistency with the existing search ---------------------------------------------------------------------------
def test_prefix_property_outside_queries_and_csr(ctx, oracle):
    E = dmodel.mixed()
    n = E.shape[0]
    D = dmodel.exact_dists(oracle, E)
    r = np.sort(D[n // 2])[12]
    with ctx.dense_index(E) as index:
        res = index.radius_search(r)
        for k in (1, 20, 64):
            idx, dist = ctx.knn(E, k)  # (between two dense-index calls: neither disturbs the other)
            for q in range(n):
                c = int((dist[q] <= r).sum())
                ix, ds = _row(res, q)
                m = min(k, ix.size)
                assert c == m and np.array_equal(idx[q, :m], ix[:m]) and \
                    np.array_equal(dist[q, :m].view(np.uint32), ds[:m].view(np.uint32)), (k, q)
        rmodel.same(index.radius_search(r), res)
        rng = np.random.default_rng(3)
        Q = np.ascontiguousarray(E[rng.choice(n, 40)] + 0.01 * rng.standard_normal((40, E.shape[1])), dtype=np.float32)
        rmodel.same(index.radius_query(Q, r), dmodel.model(oracle, E, Q)(r))
        rmodel.same(index.radius_query(E[100:231], r), _slice(res, 100, 231))


def test_index_from_csr_equals_index_from_rows(ctx):
    indptr, indices, P, F, d, E_bits = golden_embed_case("mid")
    from fedrann_amd.feature_extraction import canonical_csr
    indptr, indices = canonical_csr(indptr, indices, F)  # (the ABI wants ascending columns per row)
    ctx.projection_load(P[0], P[1], P[2], F, d)
    E = ctx.embed(indptr, indices)
    assert np.array_equal(E.view(np.uint32), E_bits)
    for r in (0.0, 0.3, 0.8):
        with ctx.dense_index(E) as a:
            want = a.radius_search(r)
        with ctx.dense_index_from_csr(indptr, indices) as b:
            got = b.radius_search(r)
            assert b.info()["n"] == E.shape[0] and b.info()["d"] == d
        rmodel.same(got, want)
    assert want[0][-1] > E.shape[0]


# ---- 5. the cap --------------------------------------------------------------------------------------------------------
def test_max_hits_refusal_and_self_cutting(ctx, oracle):
    E, r, _ = _two_segments(oracle, 8)
    E = E[:1500]
    L, h = ctx._L, ctx._h
    with ctx.dense_index(E) as index:
        full = index.radius_search(r)
        cand = index.info()["last_candidates"]
        assert cand >= full[0][-1] > 1500
        ip = np.full(1501, -1, np.int64)
        cap = int(cand) // 3
        assert L.fdr_dense_index_radius_search(h, ctypes.c_float(r), 0, 1500, cap, vp(ip.ctypes.data)) == E_ARG
        msg = L.fdr_last_error().decode()
        assert "upper" in msg and "max_hits" in msg, msg
        assert ip[0] == 0 and ip[-1] == cand > cap and np.all(np.diff(ip) >= np.diff(full[0]))  # upper bounds
        assert L.fdr_dense_index_radius_fetch(h, 0, None, None) == E_STATE  # nothing is held
        rmodel.same(index.radius_search(r), full)  # the index is as it was
        rmodel.same(index.radius_search(r, max_hits=cap), full)  # cut by the counts into pieces
        rmodel.same(index.radius_query(E[:700], r, max_hits=int(np.diff(ip)[:700].sum()) // 2), _slice(full, 0, 700))
        with pytest.raises(_lib.FedrannHipError, match="alone has"):
            index.radius_search(r, max_hits=int(np.diff(ip).max()) - 1)
        rmodel.same(index.radius_search(r), full)


# ---- 6. state ----------------------------------------------------------------------------------------------------------
def test_state_rules(ctx):
    L, h = ctx._L, ctx._h
    E = plain_rows(200, 8, 1)
    ip = np.zeros(201, np.int64)
    f = ctypes.c_float(0.2)
    ctx._check(L.fdr_dense_index_free(h), "free")
    assert L.fdr_dense_index_free(h) == 0  # (without an index: FDR_OK)
    assert L.fdr_dense_index_radius_search(h, f, 0, 1, 10, vp(ip.ctypes.data)) == E_STATE
    assert L.fdr_dense_index_radius_query(h, f, 1, vp(E.ctypes.data), 10, vp(ip.ctypes.data)) == E_STATE
    assert L.fdr_dense_index_radius_fetch(h, 0, None, None) == E_STATE
    assert L.fdr_dense_index_info(h, None, None, None, None, None, None, None) == E_STATE
    index = ctx.dense_index(E)
    assert L.fdr_dense_index_radius_fetch(h, 0, None, None) == E_STATE  # an index, no result yet
    res = index.radius_search(0.2)
    total = int(res[0][-1])
    ix, ds = np.empty(total, np.int32), np.empty(total, np.float32)
    assert L.fdr_dense_index_radius_fetch(h, total + 1, vp(ix.ctypes.data), vp(ds.ctypes.data)) == E_ARG
    assert L.fdr_dense_index_radius_fetch(h, total, vp(ix.ctypes.data), vp(ds.ctypes.data)) == 0  # (a fetch leaves it held)
    assert np.array_equal(ix, res[1]) and np.array_equal(ds.view(np.uint32), res[2].view(np.uint32))
    for bad in (1.0, -0.5, float("nan")):
        assert L.fdr_dense_index_radius_search(h, ctypes.c_float(bad), 0, 1, 10, vp(ip.ctypes.data)) == E_ARG
    assert L.fdr_dense_index_radius_fetch(h, total, vp(ix.ctypes.data), vp(ds.ctypes.data)) == E_STATE  # dropped by the call
    assert L.fdr_dense_index_radius_search(h, f, 0, 201, 10, vp(ip.ctypes.data)) == E_ARG
    assert L.fdr_dense_index_radius_search(h, f, 0, 1, 0, vp(ip.ctypes.data)) == E_ARG
    rmodel.same(index.radius_search(0.2), res)  # refused calls leave the index as it was
    # a failed build leaves none: d beyond the fp16 passes
    wide = np.zeros((4, 513), np.float32)
    assert L.fdr_dense_index_build(h, vp(wide.ctypes.data), 4, 513) == E_ARG
    assert "fp16" in L.fdr_last_error().decode()
    assert L.fdr_dense_index_info(h, None, None, None, None, None, None, None) == E_STATE
    assert L.fdr_dense_index_radius_search(h, f, 0, 1, 10, vp(ip.ctypes.data)) == E_STATE
    index2 = ctx.dense_index(E)
    with pytest.raises(_lib.FedrannHipError, match="another dense index"):
        index.radius_search(0.2)
    rmodel.same(index2.radius_search(0.2), res)
    index2.close()
    with pytest.raises(_lib.FedrannHipError, match="closed"):
        index2.info()


def test_the_two_held_radius_results_are_independent(ctx):
    """One context, a Jaccard sparse index (64 rows over 50 features) and a dense index (64 rows, d = 8), each with a
    zero row: the result a raw radius search leaves in one index is untouched by the other index's search, in either
    order, and a sparse k-NN search drops the sparse result alone."""
    L, h = ctx._L, ctx._h
    rng = np.random.default_rng(64)
    rows = [np.sort(rng.choice(50, size=rng.integers(1, 6), replace=False)).astype(np.int32) for _ in range(64)]
    rows[5] = rows[40] = np.empty(0, np.int32)  # (two empty rows: a zero query finds the other one, too)
    sp_ip = np.zeros(65, np.int64)
    sp_ip[1:] = np.cumsum([r.size for r in rows])
    sp_ix = np.concatenate(rows)
    E = plain_rows(64, 8, 64)  # (rows 3, 32 and 63 are zero)
    rs, rd = ctypes.c_float(0.7), ctypes.c_float(0.3)

    def fetch(name, total):
        ix, ds = np.empty(total, np.int32), np.empty(total, np.float32)
        rc = getattr(L, name)(h, total, vp(ix.ctypes.data), vp(ds.ctypes.data))
        return rc, ix, ds.view(np.uint32)

    with ctx.sparse_index(sp_ip, sp_ix, None, 50, metric="jaccard") as sparse, ctx.dense_index(E) as dense:
        assert sparse.info()["zero_rows"] == 2
        want = {"sparse": sparse.radius_search(rs.value), "dense": dense.radius_search(rd.value)}
        for res in want.values():
            assert res[0][-1] > 64 and np.all(np.diff(res[0]) >= 1)  # non-empty, the zero queries' rows included
        assert not np.array_equal(want["sparse"][1], want["dense"][1])
        search = {"sparse": lambda ip: L.fdr_sparse_index_radius_search(h, rs, 0, 64, 1 << 20, vp(ip.ctypes.data)),
                  "dense": lambda ip: L.fdr_dense_index_radius_search(h, rd, 0, 64, 1 << 20, vp(ip.ctypes.data))}
        for order in (("sparse", "dense"), ("dense", "sparse")):
            ips = {}
            for kind in order:  # both searches first ...
                ips[kind] = np.full(65, -1, np.int64)
                assert search[kind](ips[kind]) == 0, L.fdr_last_error().decode()
            for kind in order:  # ... then both fetches
                assert np.array_equal(ips[kind], want[kind][0])
                rc, ix, bits = fetch("fdr_%s_index_radius_fetch" % kind, int(ips[kind][-1]))
                assert rc == 0, L.fdr_last_error().decode()
                assert np.array_equal(ix, want[kind][1]) and np.array_equal(bits, want[kind][2].view(np.uint32))
        sparse.search(3)  # (a sparse call drops the sparse result; the dense one is not its business)
        assert fetch("fdr_sparse_index_radius_fetch", int(want["sparse"][0][-1]))[0] == E_STATE
        assert "no radius result" in L.fdr_last_error().decode()
        rc, ix, bits = fetch("fdr_dense_index_radius_fetch", int(want["dense"][0][-1]))
        assert rc == 0, L.fdr_last_error().decode()
        assert np.array_equal(ix, want["dense"][1]) and np.array_equal(bits, want["dense"][2].view(np.uint32))


def test_dense_and_sparse_calls_do_not_disturb_each_other(ctx, oracle):
    E = plain_rows(400, 100, 4)
    rng = np.random.default_rng(8)
    rows = [np.sort(rng.choice(50, size=rng.integers(1, 6), replace=False)).astype(np.int32) for _ in range(120)]
    sp_ip = np.zeros(121, np.int64)
    sp_ip[1:] = np.cumsum([r.size for r in rows])
    sp_ix = np.concatenate(rows)
    want = dmodel.model(oracle, E)(np.float32(0.3))
    with ctx.sparse_index(sp_ip, sp_ix, None, 50, metric="jaccard") as sparse, ctx.dense_index(E) as dense:
        s0 = sparse.search(5)
        sr0 = sparse.radius_search(0.5)
        knn0 = ctx.knn(E, 10)
        rmodel.same(dense.radius_search(0.3), want)
        s1 = sparse.search(5)
        assert np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1].view(np.uint32), s1[1].view(np.uint32))
        rmodel.same(dense.radius_search(0.3, 7, 200), _slice(want, 7, 200))
        rmodel.same(sparse.radius_search(0.5), sr0)
        knn1 = ctx.knn(E[::-1].copy(), 10)  # (another k-NN call reuses the context's scratch, not the index)
        rmodel.same(dense.radius_search(0.3), want)
        knn2 = ctx.knn(E, 10)
        assert np.array_equal(knn0[0], knn2[0]) and np.array_equal(knn0[1].view(np.uint32), knn2[1].view(np.uint32))
        assert knn1[0].shape == (400, 10)
        assert sparse.info()["n"] == 120 and dense.info()["n"] == 400
