"""RescoreRows.refine / fdr_rescore_rows_refine: the held expansion of a neighbour graph (fdr_graph_expand) scored on
the held re-score rows and cut to the k best, against the numpy models (graph.expand_rows for the candidates,
tests/_rescore_rows.py for their distances), against RescoreRows.radius on the model's expansion, and against the exact
search.  Every comparison is exact: equal indptr, equal indices, equal distance bit patterns."""
import ctypes

import numpy as np
import pytest

import _graph_rows as gr
import _radius_model as rmodel
import _rescore_rows as rr
from _rescore_rows import F, N, WHICH
from fedrann_amd import _lib
from fedrann_amd.graph import expand_rows, symmetrize_rows

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = _lib.FDR_E_ARG, _lib.FDR_E_STATE
vp = ctypes.c_void_p
KS = (1, 20, 128, 20000)
SHORT = (0, 0, 1, 20, 63, 64, 65, 128)  # row lengths within FDR_MAX_K: a fan of 128 takes every row whole


@pytest.fixture(scope="module")
def csr():
    return rr.rows()


@pytest.fixture(scope="module")
def matrices(csr, oracle):
    return rr.matrices(csr, oracle)


def _held(ctx, csr, matrices, which):
    metric, values, D = matrices[which]
    return ctx.rescore_rows(csr[0], csr[1], values, F, metric=metric), D


def cut(rows, k):
    """every row of a ragged (indptr, idx, dist) cut to its first k entries"""
    ip, ix, ds = rows
    counts = np.minimum(np.diff(ip), k)
    keep = (np.arange(ix.size) - np.repeat(ip[:-1], np.diff(ip))) < k
    out = np.zeros(ip.size, np.int64)
    np.cumsum(counts, out=out[1:])
    return out, ix[keep], ds[keep]


def keys(ix, ds):
    return (ds.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ix.astype(np.uint64)


@pytest.mark.parametrize("which", WHICH)
def test_refine_is_the_model_and_the_radius_call_on_the_models_expansion(ctx, csr, matrices, which):
    held, D = _held(ctx, csr, matrices, which)
    graph = gr.drawn(N, seed=5 + WHICH.index(which), shuffled=True)
    radii = (np.float32(1.0), rr.between(D)[0], np.float32(0.0))
    with held:
        for k in KS:
            fan = min(k, _lib.FDR_MAX_K)
            cand = expand_rows(*graph, fan)
            for r in radii:
                got = held.refine(graph, k, radius=float(r))
                rmodel.same(got, cut(rr.want(D, 0, cand[0], cand[1], r), k))
                if k in (20, 20000):
                    rmodel.same(got, cut(held.radius(cand[0], cand[1], float(r)), k))
                assert np.all(np.diff(got[0]) <= k)
        # a fan of its own, and radius == 1 with k above fan + fan^2: the plain ragged re-score of the expansion
        cand = expand_rows(*graph, 7)
        plain = held.refine(graph, 7 + 49, fan=7)
        assert np.array_equal(plain[0], cand[0])
        rmodel.same(plain, rr.want(D, 0, cand[0], cand[1], 1.0))
        rmodel.same(held.refine(graph, 3, fan=7, radius=-0.0), cut(rr.want(D, 0, cand[0], cand[1], 0.0), 3))


@pytest.mark.parametrize("which", WHICH)
def test_blocks_of_rows_give_the_same_bytes(ctx, csr, matrices, which):
    held, D = _held(ctx, csr, matrices, which)
    graph = gr.drawn(N, seed=15, shuffled=True)
    with held:
        whole = held.refine(graph, 20, radius=float(rr.between(D, 0.7)[0]))
        assert whole[0][-1] > 0
        for block in (1, 7, N):
            rmodel.same(held.refine(graph, 20, radius=float(rr.between(D, 0.7)[0]), block_rows=block), whole)
        # the default cut by the row pointer's bound: several blocks under a small cap, one row above it refused
        bound = np.minimum(np.diff(graph[0]), 20) * 21
        small = int(bound.max()) + 5
        assert bound.sum() > 3 * small
        rmodel.same(held.refine(graph, 20, radius=float(rr.between(D, 0.7)[0]), max_entries=small), whole)
        with pytest.raises(ValueError, match="one row alone"):
            held.refine(graph, 20, max_entries=int(bound.max()) - 1)


@pytest.mark.parametrize("which", ("cosine", "jaccard_sets"))
def test_reverse_is_refine_of_the_union_graph(ctx, csr, matrices, which):
    held, D = _held(ctx, csr, matrices, which)
    graph = gr.drawn(N, seed=25, shuffled=True)
    union = symmetrize_rows(*graph, "union")
    with held:
        got = held.refine(graph, 20, reverse=True)
        rmodel.same(got, held.refine(union, 20))
        cand = expand_rows(*union, 20)
        rmodel.same(got, cut(rr.want(D, 0, cand[0], cand[1], 1.0), 20))
        assert not np.array_equal(got[1], held.refine(graph, 20)[1])


@pytest.mark.parametrize("which", WHICH)
def test_a_refined_row_is_no_worse_than_its_own_list_key_by_key_and_in_recall(ctx, csr, matrices, which):
    """With a fan that takes every row whole, a row's own entries are among its candidates, so the j-th key of the
    refined row is at most the j-th key of the row's own list re-scored.  The exact search orders all rows by the same
    key, so a true neighbour inside a candidate set is within that set's first k: recall against it cannot fall."""
    metric, values, D = matrices[which]
    k = 20
    graph = gr.drawn(N, seed=35, shuffled=True, lengths=SHORT)
    assert np.diff(graph[0]).max() <= _lib.FDR_MAX_K
    with ctx.sparse_index(csr[0], csr[1], values, F, metric=metric) as index:
        exact = index.search(k)[0]
    with ctx.rescore_rows(csr[0], csr[1], values, F, metric=metric) as held:
        own = held.radius(graph[0], graph[1], 1.0)
        for kk in (k, 20000):
            got = held.refine(graph, kk, fan=_lib.FDR_MAX_K)
            better = 0
            for q in range(N):
                a = keys(got[1][got[0][q]:got[0][q + 1]], got[2][got[0][q]:got[0][q + 1]])
                b = keys(own[1][own[0][q]:own[0][q + 1]], own[2][own[0][q]:own[0][q + 1]])[:kk]
                assert a.size >= b.size and np.all(a[:b.size] <= b)
                better += int(np.any(a[:b.size] < b))
                if kk == k:
                    true = set(exact[q].tolist())
                    assert len(true & set((a & np.uint64(0xffffffff)).tolist())) >= \
                        len(true & set((b & np.uint64(0xffffffff)).tolist()))
            assert better > 0


def test_state_errors_and_the_n_mismatch(ctx, csr, matrices):
    L = _lib.load_library()
    graph = gr.drawn(N, seed=45)
    out = np.full(N + 1, -7, np.int64)

    def refine(radius=1.0, k=20):
        return L.fdr_rescore_rows_refine(ctx._h, ctypes.c_float(radius), k, vp(out.ctypes.data))
    held, D = _held(ctx, csr, matrices, "jaccard")
    with held:
        ctx.graph_free()
        assert refine() == E_STATE and b"holds no expansion" in L.fdr_last_error()
        ctx.graph_expand(graph, 20)
        for k in (0, -1):
            assert refine(k=k) == E_ARG and b"k_top" in L.fdr_last_error()
        for r in (-0.5, 1.5, float("nan")):
            assert refine(radius=r) == E_ARG and b"radius must be in [0, 1]" in L.fdr_last_error()
        assert L.fdr_rescore_rows_refine(ctx._h, ctypes.c_float(1.0), 20, None) == E_ARG
        assert np.all(out == -7)
        e = np.zeros(4, np.int32)
        assert L.fdr_rescore_rows_radius_fetch(ctx._h, 4, vp(e.ctypes.data), vp(e.ctypes.data)) == E_STATE  # nothing held
        assert refine() == 0 and out[0] == 0 and out[-1] > 0
        first = out.copy()
        assert refine(k=5) == 0 and np.all(np.diff(out) <= 5)  # the expansion stays held: any number of calls
        assert refine() == 0 and np.array_equal(out, first)
        cand = ctx.graph_expand(graph, 20)
        total = int(out[-1])
        ix, ds = np.empty(total, np.int32), np.empty(total, np.float32)
        assert L.fdr_rescore_rows_radius_fetch(ctx._h, total, vp(ix.ctypes.data), vp(ds.ctypes.data)) == 0
        rmodel.same((out, ix, ds), cut(rr.want(D, 0, cand[0], cand[1], 1.0), 20))
        # a block of rows: the expansion's own q_lo and nq
        ctx.graph_expand(graph, 20, 37, 157)
        part = np.full(121, -7, np.int64)
        assert L.fdr_rescore_rows_refine(ctx._h, ctypes.c_float(1.0), 20, vp(part.ctypes.data)) == 0
        assert np.array_equal(part, first[37:158] - first[37])
        # an expansion of a graph on other rows
        ctx.graph_expand(gr.drawn(65, seed=46), 20)
        out[:] = -7
        assert refine() == E_ARG and b"graph on 65 rows, the re-score rows are 300" in L.fdr_last_error()
        assert np.all(out == -7)
        with pytest.raises(ValueError, match="the graph has 65 rows"):
            held.refine(gr.drawn(65, seed=46), 20)
        for bad in (dict(k=0), dict(k=2 ** 31), dict(k=20, radius=1.5), dict(k=20, fan=129), dict(k=20, block_rows=0)):
            with pytest.raises(ValueError):
                held.refine(graph, **bad)
    ctx.graph_expand(graph, 20)
    assert refine() == E_STATE and b"holds no re-score rows" in L.fdr_last_error()  # the rows are gone, the expansion is not
    with pytest.raises(_lib.FedrannHipError, match="closed"):
        held.refine(graph, 20)
