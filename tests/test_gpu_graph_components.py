"""fdr_graph_components on the GPU against fedrann_amd.graph.component_labels, labels and sizes array for array, on the
graphs of tests/_component_rows.py; against the components of its own symmetrised rows; a chain (the deepest tree the
union-find can build), a hub, a giant component, a graph without entries, a k-NN graph of the library, the same bytes
on three runs, the refusals, the library's host checks, and what else the context holds."""
import ctypes
import re

import numpy as np
import pytest

import _component_rows as cr
import _graph_rows as gr
from _radius_model import same
from fedrann_amd import _lib
from fedrann_amd.graph import MODES, as_ragged, component_labels, symmetrize_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def _both_modes(ctx, graph, bounds=(None,)):
    for mode in cr.COMPONENT_MODES:
        for bound in bounds:
            cr.equal(ctx.graph_components(graph, mode, bound), component_labels(*as_ragged(graph), mode, bound))


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("bound", cr.BOUNDS)
@pytest.mark.parametrize("mode", cr.COMPONENT_MODES)
@pytest.mark.parametrize("n", [1, 2, 65, 1000])
def test_components_are_the_models(ctx, n, mode, bound, shuffled):
    graph = cr.graph_for(mode, n, seed=3, shuffled=shuffled)
    got = ctx.graph_components(graph, mode, bound)
    cr.equal(got, component_labels(*graph, mode, bound))
    if n <= 65:
        cr.equal(got, cr.brute_components(graph, mode, bound))
    elif bound is None:
        assert cr.is_rich(got[1])


@pytest.mark.parametrize("mode", cr.COMPONENT_MODES)
def test_components_of_the_symmetrised_rows(ctx, mode):
    for seed in (3, 4):
        graph = cr.graph_for(mode, 1000, seed, shuffled=True)
        for bound in cr.BOUNDS:
            want = ctx.graph_components(graph, mode, bound)
            cr.equal(ctx.graph_components(ctx.graph_symmetrize(graph, mode), "union", bound), want)
            assert want[1].size > 1


def test_a_chain(ctx):
    n = 4096
    rng = np.random.default_rng(5)
    rows = np.arange(n)
    for step in (-1, 1):  # row i lists only i - 1; as a second graph, only i + 1
        has = (rows + step >= 0) & (rows + step < n)
        ip = np.zeros(n + 1, np.int64)
        np.cumsum(has, out=ip[1:])
        idx = (rows + step)[has].astype(np.int32)
        dist = np.zeros(idx.size, np.float32)
        labels, sizes = ctx.graph_components((ip, idx, dist), "union")
        assert np.all(labels == 0) and sizes.tolist() == [n]
        labels, sizes = ctx.graph_components((ip, idx, dist), "mutual")
        assert np.array_equal(labels, rows) and np.all(sizes == 1)
        # every 64th link at 0.5, the bound at 0.25: 64 components of 64 rows
        low = np.minimum(rows[has], idx)  # the link's lower row
        dist[low % 64 == 63] = 0.5
        labels, sizes = ctx.graph_components((ip, idx, dist), "union", 0.25)
        assert np.array_equal(labels, rows // 64) and sizes.tolist() == [64] * 64
        labels, sizes = ctx.graph_components((ip, idx, dist), "union", 0.5)
        assert np.all(labels == 0) and sizes.tolist() == [n]
    # both directions, each row's two entries in a drawn order: mutual is the chain too
    listed = [[(i + s, 0.0) for s in rng.permutation([-1, 1]) if 0 <= i + s < n] for i in range(n)]
    labels, sizes = ctx.graph_components(gr.from_rows(listed), "mutual")
    assert np.all(labels == 0) and sizes.tolist() == [n]


def test_a_hub(ctx):
    n = 20000
    ip = np.arange(n + 1, dtype=np.int64)
    idx = np.full(n, n - 1, np.int32)  # every row lists row n - 1 only (the hub itself too: a self entry)
    dist = np.zeros(n, np.float32)
    labels, sizes = ctx.graph_components((ip, idx, dist), "union")
    assert np.all(labels == 0) and sizes.tolist() == [n]  # one component, whose root is row 0
    # two hubs, h and n - 1, each listed by its half of the rows
    h = n // 2 - 1
    idx[:h + 1] = h
    labels, sizes = ctx.graph_components((ip, idx, dist), "union")
    assert np.array_equal(labels, (np.arange(n) > h).astype(np.int32)) and sizes.tolist() == [h + 1, n - h - 1]
    cr.equal((labels, sizes), component_labels(ip, idx, dist, "union"))
    # ... and one entry between two leaf rows joins them
    rows = [[(int(t), 0.0)] for t in idx]
    rows[17].append((n - 5, 0.25))
    joined = gr.from_rows(rows)
    labels, sizes = ctx.graph_components(joined, "union")
    assert np.all(labels == 0) and sizes.tolist() == [n]
    cr.equal(ctx.graph_components(joined, "union", 0.125), component_labels(*joined, "union", 0.125))
    assert ctx.graph_components(joined, "union", 0.125)[1].tolist() == [h + 1, n - h - 1]


def test_a_giant_component_among_small_ones(ctx):
    graph = cr.graph_for("union", 5000, seed=3, shuffled=True)
    got = ctx.graph_components(graph, "union")
    cr.equal(got, component_labels(*graph, "union"))
    assert got[1].max() > 2500 and np.sum(got[1] == 1) > 500  # whole waves of one root, and waves of many


def test_a_graph_without_entries(ctx):
    L = _lib.load_library()
    empty = (np.zeros(66, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    for mode in cr.COMPONENT_MODES:
        got = ctx.graph_components(empty, mode)
        cr.equal(got, component_labels(*empty, mode))
        assert got[0].tolist() == list(range(65)) and got[1].tolist() == [1] * 65
        labels, sizes, found = np.full(65, -7, np.int32), np.full(65, -7, np.int64), ctypes.c_int64(-7)
        assert L.fdr_graph_components(ctx._h, MODES[mode], 65, empty[0].ctypes.data, None, None, np.float32(0.5),
                                      labels.ctypes.data, sizes.ctypes.data, ctypes.addressof(found)) == 0
        assert found.value == 65 and labels.tolist() == list(range(65)) and np.all(sizes == 1)
    only_self = gr.from_rows([[(0, 0.0)], [(1, 0.5)], []])  # entries, and still nothing joined
    _both_modes(ctx, only_self)
    assert ctx.graph_components(only_self)[0].tolist() == [0, 1, 2]


def test_asymmetric_distances_and_self_entries(ctx):
    graph = gr.asymmetric()
    _both_modes(ctx, graph, (None, 0.5, 0.3, 0.2, 0.125, 0.1, gr.TINY, 0.0, float("inf")))
    assert ctx.graph_components(graph, "mutual", 0.3)[0].tolist() == [0, 0, 0, 0, 1]
    assert ctx.graph_components(graph, "mutual", 0.2)[0].tolist() == [0, 1, 1, 0, 2]
    one_way = gr.from_rows([[(3, gr.TINY)], [], [], [], []])
    assert ctx.graph_components(one_way, "union", 0.0)[0].tolist() == [0, 1, 2, 3, 4]
    assert ctx.graph_components(one_way, "union", gr.TINY)[0].tolist() == [0, 1, 2, 0, 3]


def test_a_knn_graph_of_the_library(ctx):
    from fedrann_amd.synth import synth
    from fedrann_amd import feature_extraction as fx
    from fedrann_amd.precompute import build_precompute_matrix
    s = synth(500, seed=5, m=60, doubling=True)  # 1000 rows: every read on both strands
    P = fx._projection_csr(build_precompute_matrix(s["counts"], 64, n_features=s["n_features"]))
    ctx.projection_load(P.indptr, P.indices, P.data, s["n_features"], 64)
    idx, dist = ctx.knn(ctx.embed(s["indptr"], s["indices"]), 20)
    assert idx.shape == (1000, 20)
    cut = float(np.median(dist[:, 3]))
    _both_modes(ctx, (idx, dist), (None, cut, 0.0))
    assert ctx.graph_components((idx, dist), "mutual", cut)[1].size > ctx.graph_components((idx, dist), "union")[1].size


def test_the_same_bytes_every_time(ctx):
    graph, other = cr.graph_for("mutual", 1000, seed=4, shuffled=True), cr.graph_for("union", 300, seed=3, shuffled=True)
    for mode in cr.COMPONENT_MODES:
        first = ctx.graph_components(graph, mode, 0.25)
        cr.equal(ctx.graph_components(graph, mode, 0.25), first)
        ctx.graph_components(other, mode)
        cr.equal(ctx.graph_components(graph, mode, 0.25), first)
        cr.equal(ctx.graph_components(cr.shuffle_rows(graph, 9), mode, 0.25), first)  # the entries' order cannot show


def _raw(ctx, graph, mode="union", bound=np.inf, fill=-7, found=-7):
    """The raw call on prefilled outputs: (rc, labels, sizes, n_components)."""
    L = _lib.load_library()
    ip, ix, ds = graph
    labels, sizes, c = np.full(ip.size - 1, fill, np.int32), np.full(ip.size - 1, fill, np.int64), ctypes.c_int64(found)
    rc = L.fdr_graph_components(ctx._h, MODES[mode], ip.size - 1, ip.ctypes.data, ix.ctypes.data, ds.ctypes.data,
                                np.float32(bound), labels.ctypes.data, sizes.ctypes.data, ctypes.addressof(c))
    return rc, labels, sizes, c.value


def _refused(ctx, graph, match):
    """FDR_E_ARG, the symmetrise's words, nothing written."""
    L = _lib.load_library()
    for mode in cr.COMPONENT_MODES:
        for bound in (np.inf, 0.0):
            rc, labels, sizes, found = _raw(ctx, graph, mode, bound)
            assert rc == _lib.FDR_E_ARG and np.all(labels == -7) and np.all(sizes == -7) and found == -7
            assert re.search("graph_components: " + match, L.fdr_last_error().decode()), L.fdr_last_error()
        with pytest.raises(_lib.FedrannHipError, match=match):
            ctx.graph_components(graph, mode)
        with pytest.raises(ValueError, match=match):  # the model names the same row and rule
            component_labels(*graph, mode)


def _edited(graph, fn):
    out = tuple(a.copy() for a in graph)
    fn(*out)
    return out


def test_refusals_write_nothing_and_the_next_call_is_correct(ctx):
    good = gr.drawn(65, seed=31, shuffled=True, lengths=(5, 63, 64, 65))
    ip = good[0]
    last = int(ip[65] - ip[64]) - 1  # the last entry of the last row
    over = next(r for r in range(1, 65) if int(ip[r]) // 64 != (int(ip[r + 1]) - 1) // 64 and int(ip[r]) % 64)
    edge = 64 * (int(ip[over]) // 64 + 1) - int(ip[over])  # row `over`'s first entry in the next 64 of the walk
    bounds = (None, 0.25)
    _both_modes(ctx, good, bounds)

    def index(r, j, v):
        return lambda _, ix, ds: ix.__setitem__(int(ip[r]) + j, v)

    def distance(r, j, v):
        return lambda _, ix, ds: ds.__setitem__(int(ip[r]) + j, v)

    def twice(r, a, b):
        return lambda _, ix, ds: ix.__setitem__(int(ip[r]) + b, ix[int(ip[r]) + a])
    for r, j in ((0, 0), (64, last), (over, edge)):
        _refused(ctx, _edited(good, index(r, j, -3)), "row %d: an index outside" % r)
        _refused(ctx, _edited(good, index(r, j, 65)), "row %d: an index outside" % r)
        _refused(ctx, _edited(good, distance(r, j, -0.5)), "row %d: a distance that is negative or NaN" % r)
        _refused(ctx, _edited(good, distance(r, j, np.nan)), "row %d: a distance that is negative or NaN" % r)
        _both_modes(ctx, good, bounds)
    _refused(ctx, _edited(good, distance(3, 1, -0.0)), "row 3: a distance that is negative or NaN")
    _refused(ctx, _edited(good, twice(0, 0, 1)), "row 0: an index listed twice")
    _refused(ctx, _edited(good, twice(64, 0, last)), "row 64: an index listed twice")
    _refused(ctx, _edited(good, twice(over, edge - 1, edge)), "row %d: an index listed twice" % over)
    several = _edited(_edited(_edited(good, twice(5, 0, 2)), distance(5, 1, np.nan)), index(40, 0, -2))
    _refused(ctx, several, "row 5: a distance")  # the smallest (row, rule)
    _refused(ctx, _edited(several, index(5, 3, 99)), "row 5: an index outside")
    _both_modes(ctx, good, bounds)


def test_the_limits_in_the_library(ctx):
    L = _lib.load_library()
    fn = L.fdr_graph_components
    ip, ix, ds = gr.drawn(2, seed=61, lengths=(2,))
    labels, sizes, found = np.full(2, -7, np.int32), np.full(2, -7, np.int64), ctypes.c_int64(-7)
    p = [a.ctypes.data for a in (ip, ix, ds, labels, sizes)] + [ctypes.addressof(found)]
    inf, bad = np.float32(np.inf), _lib.FDR_E_ARG
    assert fn(ctx._h, 0, 2, p[0], p[1], p[2], inf, p[3], p[4], p[5]) == 0 and found.value == 1
    assert labels.tolist() == [0, 0] and sizes.tolist() == [2, -7]  # the first C sizes; the rest as they were
    labels[:] = -7
    assert fn(ctx._h, 1, 2, p[0], p[1], p[2], inf, p[3], None, p[5]) == 0 and labels.tolist() == [0, 0]  # no sizes wanted
    labels[:], sizes[:], found.value = -7, -7, -7
    assert fn(ctx._h, 0, 2, None, p[1], p[2], inf, p[3], p[4], p[5]) == bad  # null pointers
    assert fn(ctx._h, 0, 2, p[0], None, p[2], inf, p[3], p[4], p[5]) == bad
    assert fn(ctx._h, 0, 2, p[0], p[1], None, inf, p[3], p[4], p[5]) == bad
    assert fn(ctx._h, 0, 2, p[0], p[1], p[2], inf, None, p[4], p[5]) == bad
    assert fn(ctx._h, 0, 2, p[0], p[1], p[2], inf, p[3], p[4], None) == bad
    assert fn(ctx._h, 0, 0, p[0], p[1], p[2], inf, p[3], p[4], p[5]) == bad and b"n (0)" in L.fdr_last_error()
    assert fn(ctx._h, 0, -1, p[0], p[1], p[2], inf, p[3], p[4], p[5]) == bad
    assert fn(ctx._h, 0, 2 ** 31, p[0], p[1], p[2], inf, p[3], p[4], p[5]) == bad
    assert fn(ctx._h, 2, 2, p[0], p[1], p[2], inf, p[3], p[4], p[5]) == bad and b"mode 2" in L.fdr_last_error()  # transpose
    assert fn(ctx._h, 3, 2, p[0], p[1], p[2], inf, p[3], p[4], p[5]) == bad and b"mode 3" in L.fdr_last_error()
    assert fn(ctx._h, -1, 2, p[0], p[1], p[2], inf, p[3], p[4], p[5]) == bad
    for bound in (np.nan, -1.0, -0.0, -np.inf):
        assert fn(ctx._h, 0, 2, p[0], p[1], p[2], np.float32(bound), p[3], p[4], p[5]) == bad
        assert b"max_distance" in L.fdr_last_error()
    for broken in ([0, 3, 2], [1, 2, 4], [0, -1, 4]):  # a decreasing indptr, one that does not start at 0
        b = np.array(broken, np.int64)
        assert fn(ctx._h, 0, 2, b.ctypes.data, p[1], p[2], inf, p[3], p[4], p[5]) == bad
    big = np.array([0, 2 ** 31], np.int64)  # 2^31 entries by the indptr alone: refused before anything is read
    assert fn(ctx._h, 0, 1, big.ctypes.data, p[1], p[2], inf, p[3], p[4], p[5]) == bad and b"2^31" in L.fdr_last_error()
    assert np.all(labels == -7) and np.all(sizes == -7) and found.value == -7  # no refusal wrote anything
    with pytest.raises(ValueError, match="union or mutual"):
        ctx.graph_components((ip, ix, ds), "transpose")
    with pytest.raises(ValueError, match="max_distance"):
        ctx.graph_components((ip, ix, ds), "union", -0.0)


def test_what_else_the_context_holds_stays_as_it_is(ctx):
    from fedrann_amd.synth import synth
    s = synth(300, seed=9, doubling=True)
    L = _lib.load_library()
    graph = cr.graph_for("mutual", 300, seed=3, shuffled=True)
    larger = cr.graph_for("union", 1000, seed=4, shuffled=True)
    held = symmetrize_rows(*graph, "union")
    with ctx.sparse_index(s["indptr"], s["indices"], None, s["n_features"], metric="jaccard") as index, \
            ctx.dense_index(np.random.default_rng(2).standard_normal((600, 64)).astype(np.float32)) as dense:
        before = index.radius_search(0.9, 0, 100)
        dense_before = dense.radius_search(0.9, 0, 100)
        # radius calls whose results are still held by the context: counts taken, hits not yet fetched
        ip = np.full(101, -1, np.int64)
        assert L.fdr_sparse_index_radius_search(ctx._h, np.float32(0.9), 0, 100, 1 << 26, ip.ctypes.data) == 0
        dip = np.full(101, -1, np.int64)
        assert L.fdr_dense_index_radius_search(ctx._h, np.float32(0.9), 0, 100, 1 << 26, dip.ctypes.data) == 0
        assert np.array_equal(ip, before[0]) and np.array_equal(dip, dense_before[0])
        # ... and a symmetrised graph, counted and not yet fetched
        out = np.full(301, -7, np.int64)
        assert L.fdr_graph_symmetrize(ctx._h, 0, 300, graph[0].ctypes.data, graph[1].ctypes.data, graph[2].ctypes.data,
                                      1 << 27, out.ctypes.data) == 0
        trace, info = ctx.last_knn_trace(), index.info()
        _both_modes(ctx, larger, (None, 0.25))  # a larger graph through the shared input arrays
        _both_modes(ctx, graph, (None, 0.0))
        total = int(out[-1])
        ix, ds = np.empty(total, np.int32), np.empty(total, np.float32)
        assert L.fdr_graph_symmetrize_fetch(ctx._h, total, ix.ctypes.data, ds.ctypes.data) == 0
        same((out, ix, ds), held)
        total = int(ip[-1])
        ix, ds = np.empty(total, np.int32), np.empty(total, np.float32)
        assert L.fdr_sparse_index_radius_fetch(ctx._h, total, ix.ctypes.data, ds.ctypes.data) == 0
        same((ip, ix, ds), before)
        total = int(dip[-1])
        ix, ds = np.empty(total, np.int32), np.empty(total, np.float32)
        assert L.fdr_dense_index_radius_fetch(ctx._h, total, ix.ctypes.data, ds.ctypes.data) == 0
        same((dip, ix, ds), dense_before)
        assert ctx.last_knn_trace() == trace and index.info() == info
        ctx.graph_free()
        _both_modes(ctx, larger)  # after graph_free the buffers grow again
        same(index.radius_search(0.9, 0, 100), before)
        same(dense.radius_search(0.9, 0, 100), dense_before)
