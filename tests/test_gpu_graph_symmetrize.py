"""fdr_graph_symmetrize on the GPU against fedrann_amd.graph.symmetrize_rows, bit for bit, on ragged graphs where the
index decides most positions (tests/_graph_rows.py): union, mutual and transposed rows, sorted and shuffled input rows,
a hub, one long row, asymmetric distances, the refusals, the cap, the fetch, the limits, and what else the context
holds."""
import re

import numpy as np
import pytest

import _graph_rows as gr
from _radius_model import same
from fedrann_amd import _lib
from fedrann_amd.graph import MODES, as_ragged, symmetrize_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def _all_modes(ctx, graph):
    for mode in gr.MODES:
        same(ctx.graph_symmetrize(graph, mode), symmetrize_rows(*as_ragged(graph), mode))


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("mode", gr.MODES)
@pytest.mark.parametrize("n", [1, 2, 65, 1000])
def test_symmetrize_is_the_model_bit_for_bit(ctx, n, mode, shuffled):
    graph = gr.drawn(n, seed=10 * n + shuffled, shuffled=shuffled)
    got = ctx.graph_symmetrize(graph, mode)
    same(got, symmetrize_rows(*graph, mode))
    if n <= 65:
        same(got, gr.brute(graph, mode))


def test_a_knn_graph_of_the_library_and_its_overlaps_file(ctx, tmp_path):
    from fedrann_amd.synth import synth
    from fedrann_amd import feature_extraction as fx
    from fedrann_amd.precompute import build_precompute_matrix
    s = synth(500, seed=5, m=60, doubling=True)  # 1000 rows: every read on both strands
    P = fx._projection_csr(build_precompute_matrix(s["counts"], 64, n_features=s["n_features"]))
    ctx.projection_load(P.indptr, P.indices, P.data, s["n_features"], 64)
    idx, dist = ctx.knn(ctx.embed(s["indptr"], s["indices"]), 20)
    assert idx.shape == (1000, 20) and np.any(idx == np.arange(1000)[:, None])  # self entries included
    _all_modes(ctx, (idx, dist))
    union = ctx.graph_symmetrize((idx, dist), "union")
    assert union[1].size > idx.size  # (some lists are not reciprocated)
    name_off, names = _lib.pack_names(s["names"])
    strands = np.asarray(s["strands"], np.uint8)
    files = []
    for tag, rows in (("got", union), ("want", symmetrize_rows(*as_ragged((idx, dist)), "union"))):
        files.append(tmp_path / (tag + ".tsv"))
        assert _lib.overlaps_write_csr(str(files[-1]), *rows, name_off, names, strands) > 20 * 1000 - 1000
    assert files[0].read_bytes() == files[1].read_bytes()


def test_a_hub_listed_by_every_row(ctx):
    n = 5000
    rng = np.random.default_rng(11)
    rows = [[(7, float(rng.choice(gr.LEVELS)))] for _ in range(n)]
    rows[7] = [(1, 0.25), (4000, 0.0), (4999, 0.5)]
    graph = gr.from_rows(rows)
    t = ctx.graph_symmetrize(graph, "transpose")
    same(t, symmetrize_rows(*graph, "transpose"))
    lo, hi = int(t[0][7]), int(t[0][8])
    assert hi - lo == n - 1  # every row but row 7 itself
    key = (gr.bits(t[2][lo:hi]).astype(np.uint64) << np.uint64(32)) | t[1][lo:hi].astype(np.uint64)
    assert np.all(key[1:] > key[:-1])
    rows[7].append((7, 0.0))  # ... and with its own entry: all 5000
    graph = gr.from_rows(rows)
    t = ctx.graph_symmetrize(graph, "transpose")
    same(t, symmetrize_rows(*graph, "transpose"))
    assert int(t[0][8] - t[0][7]) == n
    _all_modes(ctx, graph)


def test_one_long_row_among_short_ones(ctx):
    n = 6000
    rng = np.random.default_rng(12)
    rows = [[(int(t), float(rng.choice(gr.LEVELS))) for t in rng.permutation(n)[:3]] for _ in range(n)]
    rows[0] = [(int(t), float(rng.choice(gr.LEVELS))) for t in rng.permutation(n)[:4096]]
    graph = gr.from_rows(rows)
    assert int(graph[0][1]) == 4096
    _all_modes(ctx, graph)


def test_asymmetric_distances_and_self_entries(ctx):
    graph = gr.asymmetric()
    _all_modes(ctx, graph)
    for mode in gr.MODES:
        same(ctx.graph_symmetrize(graph, mode), gr.brute(graph, mode))


def test_the_same_bytes_every_time(ctx):
    graph, other = gr.drawn(1000, seed=21, shuffled=True), gr.drawn(300, seed=22, shuffled=True)
    for mode in gr.MODES:
        first = ctx.graph_symmetrize(graph, mode)
        same(ctx.graph_symmetrize(graph, mode), first)
        ctx.graph_symmetrize(other, mode)
        same(ctx.graph_symmetrize(graph, mode), first)


def _raw(ctx, graph, mode="union", max_entries=1 << 27, fill=-7):
    """The raw count call on a prefilled indptr_out: (rc, indptr_out)."""
    L = _lib.load_library()
    ip, ix, ds = graph
    out = np.full(ip.size, fill, np.int64)
    rc = L.fdr_graph_symmetrize(ctx._h, MODES[mode], ip.size - 1, ip.ctypes.data, ix.ctypes.data, ds.ctypes.data,
                                max_entries, out.ctypes.data)
    return rc, out


def _refused(ctx, graph, match):
    """FDR_E_ARG, the message, nothing written, nothing held."""
    L = _lib.load_library()
    for mode in gr.MODES:
        rc, out = _raw(ctx, graph, mode)
        assert rc == _lib.FDR_E_ARG and np.all(out == -7)
        assert re.search(match, L.fdr_last_error().decode()), L.fdr_last_error()
        e = np.full(4, -7, np.int32)
        assert L.fdr_graph_symmetrize_fetch(ctx._h, 4, e.ctypes.data, e.ctypes.data) == _lib.FDR_E_STATE
        assert np.all(e == -7)
    with pytest.raises(_lib.FedrannHipError, match=match):
        ctx.graph_symmetrize(graph)
    with pytest.raises(ValueError, match=match):  # the model names the same row and rule
        symmetrize_rows(*graph, "union")


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
    _all_modes(ctx, good)

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
        _all_modes(ctx, good)
    _refused(ctx, _edited(good, distance(3, 1, -0.0)), "row 3: a distance that is negative or NaN")
    _refused(ctx, _edited(good, twice(0, 0, 1)), "row 0: an index listed twice")
    _refused(ctx, _edited(good, twice(64, 0, last)), "row 64: an index listed twice")
    _refused(ctx, _edited(good, twice(over, edge - 1, edge)), "row %d: an index listed twice" % over)
    several = _edited(_edited(_edited(good, twice(5, 0, 2)), distance(5, 1, np.nan)), index(40, 0, -2))
    _refused(ctx, several, "row 5: a distance")  # the smallest (row, rule)
    _refused(ctx, _edited(several, index(5, 3, 99)), "row 5: an index outside")
    _all_modes(ctx, good)


def test_the_cap(ctx):
    graph = gr.drawn(300, seed=41, shuffled=True)
    L = _lib.load_library()
    for mode in gr.MODES:
        want = symmetrize_rows(*graph, mode)
        total = int(want[0][-1])
        same(ctx.graph_symmetrize(graph, mode, max_entries=total), want)
        rc, out = _raw(ctx, graph, mode, max_entries=total - 1)
        assert rc == _lib.FDR_E_ARG and np.array_equal(out, want[0])  # indptr_out holds the counts
        msg = L.fdr_last_error().decode()
        assert "%d entries exceed max_entries = %d" % (total, total - 1) in msg and "indptr_out holds the counts" in msg
        e = np.full(4, -7, np.int32)
        assert L.fdr_graph_symmetrize_fetch(ctx._h, total, e.ctypes.data, e.ctypes.data) == _lib.FDR_E_STATE
        with pytest.raises(_lib.FedrannHipError, match="exceed max_entries"):
            ctx.graph_symmetrize(graph, mode, max_entries=total - 1)


def test_fetch_misuse(ctx):
    graph = gr.drawn(65, seed=51)
    L = _lib.load_library()
    rc, out = _raw(ctx, graph, "union")
    total = int(out[-1])
    assert rc == 0 and total > 0
    ix, ds = np.full(total + 1, -7, np.int32), np.full(total + 1, -7.0, np.float32)
    for wrong in (total - 1, total + 1, 0):
        assert L.fdr_graph_symmetrize_fetch(ctx._h, wrong, ix.ctypes.data, ds.ctypes.data) == _lib.FDR_E_ARG
        assert ("entries = %d, the held result has %d" % (wrong, total)).encode() in L.fdr_last_error()
    assert L.fdr_graph_symmetrize_fetch(ctx._h, total, None, ds.ctypes.data) == _lib.FDR_E_ARG
    assert np.all(ix == -7) and np.all(ds == -7.0)
    assert L.fdr_graph_symmetrize_fetch(ctx._h, total, ix.ctypes.data, ds.ctypes.data) == 0  # (still held; twice is fine)
    same((out, ix[:total].copy(), ds[:total].copy()), symmetrize_rows(*graph, "union"))
    assert ix[total] == -7
    ctx.graph_free()
    assert L.fdr_graph_symmetrize_fetch(ctx._h, total, ix.ctypes.data, ds.ctypes.data) == _lib.FDR_E_STATE
    assert b"holds no symmetrised graph" in L.fdr_last_error()
    ctx.graph_free()  # (with nothing to free)
    _all_modes(ctx, graph)


def test_the_limits_in_the_library(ctx):
    L = _lib.load_library()
    fn = L.fdr_graph_symmetrize
    ip, ix, ds = gr.drawn(2, seed=61, lengths=(2,))
    out = np.full(3, -7, np.int64)
    p = [a.ctypes.data for a in (ip, ix, ds, out)]
    assert fn(ctx._h, 0, 2, p[0], p[1], p[2], 1 << 20, p[3]) == 0 and out[-1] > 0
    out[:] = -7
    bad = _lib.FDR_E_ARG
    assert fn(ctx._h, 0, 2, None, p[1], p[2], 1 << 20, p[3]) == bad  # null pointers
    assert fn(ctx._h, 0, 2, p[0], None, p[2], 1 << 20, p[3]) == bad
    assert fn(ctx._h, 0, 2, p[0], p[1], None, 1 << 20, p[3]) == bad
    assert fn(ctx._h, 0, 2, p[0], p[1], p[2], 1 << 20, None) == bad
    assert fn(ctx._h, 0, 0, p[0], p[1], p[2], 1 << 20, p[3]) == bad and b"n (0)" in L.fdr_last_error()
    assert fn(ctx._h, 0, -1, p[0], p[1], p[2], 1 << 20, p[3]) == bad
    assert fn(ctx._h, 0, 2 ** 31, p[0], p[1], p[2], 1 << 20, p[3]) == bad
    assert fn(ctx._h, 3, 2, p[0], p[1], p[2], 1 << 20, p[3]) == bad and b"mode 3" in L.fdr_last_error()
    assert fn(ctx._h, -1, 2, p[0], p[1], p[2], 1 << 20, p[3]) == bad
    assert fn(ctx._h, 0, 2, p[0], p[1], p[2], 0, p[3]) == bad and b"max_entries" in L.fdr_last_error()
    assert fn(ctx._h, 0, 2, p[0], p[1], p[2], 2 ** 31, p[3]) == bad
    for broken in ([0, 3, 2], [1, 2, 4], [0, -1, 4]):  # a decreasing indptr, one that does not start at 0
        b = np.array(broken, np.int64)
        assert fn(ctx._h, 0, 2, b.ctypes.data, p[1], p[2], 1 << 20, p[3]) == bad
    big = np.array([0, 2 ** 31], np.int64)  # 2^31 entries by the indptr alone: refused before anything is read
    assert fn(ctx._h, 0, 1, big.ctypes.data, p[1], p[2], 1 << 20, p[3]) == bad and b"2^31" in L.fdr_last_error()
    assert np.all(out == -7)  # no refusal wrote anything
    e = np.zeros(1, np.int32)
    assert L.fdr_graph_symmetrize_fetch(ctx._h, int(4), e.ctypes.data, e.ctypes.data) == _lib.FDR_E_STATE  # nothing held


def test_a_graph_without_entries(ctx):
    L = _lib.load_library()
    empty = (np.zeros(66, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    for mode in gr.MODES:
        got = ctx.graph_symmetrize(empty, mode)
        assert got[0].tolist() == [0] * 66 and got[1].size == got[2].size == 0
        same(got, symmetrize_rows(*empty, mode))
        out = np.full(66, -7, np.int64)
        assert L.fdr_graph_symmetrize(ctx._h, MODES[mode], 65, empty[0].ctypes.data, None, None, 1, out.ctypes.data) == 0
        assert np.all(out == 0)
        assert L.fdr_graph_symmetrize_fetch(ctx._h, 0, None, None) == 0  # an empty result is held
        assert L.fdr_graph_symmetrize_fetch(ctx._h, 1, None, None) == _lib.FDR_E_ARG
    one_way = gr.from_rows([[(1, 0.5)], [(2, 0.5)], []])  # mutual rows of a graph without a reciprocated pair
    got = ctx.graph_symmetrize(one_way, "mutual")
    assert got[0].tolist() == [0, 0, 0, 0] and got[1].size == 0
    same(ctx.graph_symmetrize(one_way, "union"), symmetrize_rows(*one_way, "union"))


def test_the_indexes_their_held_results_and_the_trace_stay_as_they_are(ctx):
    from fedrann_amd.synth import synth
    s = synth(300, seed=9, doubling=True)
    L = _lib.load_library()
    graph = gr.drawn(300, seed=71, shuffled=True)
    want = symmetrize_rows(*graph, "union")
    with ctx.sparse_index(s["indptr"], s["indices"], None, s["n_features"], metric="jaccard") as index:
        same(ctx.graph_symmetrize(graph), want)  # a call before ...
        before = index.radius_search(0.9, 0, 100)
        knn = index.search(10, 0, 100)
        # a radius call whose result is still held by the context: counts taken, hits not yet fetched
        ip = np.full(101, -1, np.int64)
        assert L.fdr_sparse_index_radius_search(ctx._h, np.float32(0.9), 0, 100, 1 << 26, ip.ctypes.data) == 0
        assert np.array_equal(ip, before[0])
        trace, info = ctx.last_knn_trace(), index.info()  # (the radius call's own record)
        same(ctx.graph_symmetrize(graph), want)  # ... one between the search and its fetch ...
        total = int(ip[-1])
        idx, dist = np.empty(total, np.int32), np.empty(total, np.float32)
        assert L.fdr_sparse_index_radius_fetch(ctx._h, total, idx.ctypes.data, dist.ctypes.data) == 0
        same((ip, idx, dist), before)
        assert ctx.last_knn_trace() == trace and index.info() == info
        same(ctx.graph_symmetrize(graph, "mutual"), symmetrize_rows(*graph, "mutual"))  # ... and one after
        ctx.graph_free()
        same(index.radius_search(0.9, 0, 100), before)
        got = index.search(10, 0, 100)
        assert np.array_equal(got[0], knn[0]) and np.array_equal(got[1].view(np.uint32), knn[1].view(np.uint32))
        # the library's own rows through the call: a radius result is a ragged graph once its rows cover all reads
        whole = index.radius_search(0.9)
        _all_modes(ctx, whole)
