"""fdr_graph_expand on the GPU against fedrann_amd.graph.expand_rows, byte for byte, on the symmetrise tests' graphs
(tests/_graph_rows.py): every fan at the wave and FDR_MAX_K edges, whole graphs and row ranges, a hub, the refusals, the
cap, the fetch, and what else the context holds."""
import re

import numpy as np
import pytest

import _expand_rows as er
import _graph_rows as gr
from _radius_model import same
from fedrann_amd import _lib
from fedrann_amd.graph import expand_rows, symmetrize_rows

pytestmark = pytest.mark.gpu

FANS = (1, 2, 63, 64, 65, 128)


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("n", [1, 2, 65, 700])
def test_expand_is_the_model_byte_for_byte(ctx, n, shuffled):
    graph = gr.drawn(n, seed=10 * n + shuffled, shuffled=shuffled)
    for fan in FANS:
        got = ctx.graph_expand(graph, fan)
        er.same(got, expand_rows(*graph, fan))
        if n <= 65:
            er.same(got, er.brute(graph, fan))


def test_row_ranges_that_start_and_end_inside_a_64_entry_boundary(ctx):
    graph = gr.drawn(700, seed=14, shuffled=True)
    ip = graph[0]
    inside = [r for r in range(1, 700) if int(ip[r]) % 64]  # rows whose first entry is no multiple of 64
    assert len(inside) > 10
    for fan in (2, 64, 128):
        whole = expand_rows(*graph, fan)
        for lo, hi in ((inside[0], inside[5]), (inside[3], inside[3] + 1), (inside[-4], 700), (0, inside[2]), (5, 5),
                       (699, 700), (700, 700)):
            got = ctx.graph_expand(graph, fan, lo, hi)
            er.same(got, (whole[0][lo:hi + 1] - whole[0][lo], whole[1][whole[0][lo]:whole[0][hi]]))


def test_asymmetric_distances_and_self_entries(ctx):
    graph = gr.asymmetric()
    for fan in (1, 2, 3, 128):
        er.same(ctx.graph_expand(graph, fan), er.brute(graph, fan))
    twice = gr.from_rows([[(1, 0.0), (1, 0.0), (2, 0.25)], [(3, 0.0)], [(4, 0.0)], [], []])
    for fan in (1, 2, 3):  # an index twice in a row: two places of the fan, out once, not refused
        er.same(ctx.graph_expand(twice, fan), er.brute(twice, fan))
    assert ctx.graph_expand(twice, 2, 0, 1)[1].tolist() == [1, 3]


def test_the_same_bytes_every_time(ctx):
    graph, other = gr.drawn(700, seed=21, shuffled=True), gr.drawn(300, seed=22, shuffled=True)
    first = ctx.graph_expand(graph, 65)
    er.same(ctx.graph_expand(graph, 65), first)
    ctx.graph_expand(other, 128)
    er.same(ctx.graph_expand(graph, 65), first)


def test_a_hub_and_rows_at_the_upper_bound(ctx):
    """Every row lists row 0 first and 299 more; row 0 lists 300 rows: at fan 128 every row gathers 128 + 128^2."""
    n = 320
    rng = np.random.default_rng(31)
    rows = []
    for r in range(n):
        others = rng.permutation(np.arange(1, n))[:299]
        rows.append([(0, 0.0)] + [(int(t), float(rng.choice(gr.LEVELS[1:]))) for t in others])
    graph = gr.from_rows(rows)
    got = ctx.graph_expand(graph, 128)
    er.same(got, expand_rows(*graph, 128))
    assert np.all(got[1][got[0][:-1]] == 0)  # every row names the hub
    er.same(ctx.graph_expand(graph, 128, 7, 9), er.brute(graph, 128, 7, 9))


def test_a_graph_without_entries(ctx):
    L = _lib.load_library()
    empty = (np.zeros(66, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    got = ctx.graph_expand(empty, 20)
    assert got[0].tolist() == [0] * 66 and got[1].size == 0
    er.same(got, expand_rows(*empty, 20))
    out = np.full(11, -7, np.int64)
    assert L.fdr_graph_expand(ctx._h, 65, empty[0].ctypes.data, None, None, 20, 5, 10, 1, out.ctypes.data) == 0
    assert np.all(out == 0)
    assert L.fdr_graph_expand_fetch(ctx._h, 0, None) == 0  # an empty result is held
    assert L.fdr_graph_expand_fetch(ctx._h, 1, None) == _lib.FDR_E_ARG
    lonely = gr.from_rows([[], [(0, 0.5)], []])  # rows without entries among rows with some
    er.same(ctx.graph_expand(lonely, 3), er.brute(lonely, 3))
    er.same(ctx.graph_expand(lonely, 3, 2, 3), er.brute(lonely, 3, 2, 3))


def _raw(ctx, graph, fan, lo=0, hi=None, max_entries=1 << 27, fill=-7):
    L = _lib.load_library()
    ip, ix, ds = graph
    n = ip.size - 1
    hi = n if hi is None else hi
    out = np.full(hi - lo + 1, fill, np.int64)
    rc = L.fdr_graph_expand(ctx._h, n, ip.ctypes.data, ix.ctypes.data, ds.ctypes.data, fan, lo, hi - lo, max_entries,
                            out.ctypes.data)
    return rc, out


def _nothing_held(ctx):
    L = _lib.load_library()
    e = np.full(4, -7, np.int32)
    assert L.fdr_graph_expand_fetch(ctx._h, 4, e.ctypes.data) == _lib.FDR_E_STATE
    assert b"holds no expansion" in L.fdr_last_error() and np.all(e == -7)


def test_the_cap_leaves_the_counts_and_holds_nothing(ctx):
    graph = gr.drawn(300, seed=41, shuffled=True)
    L = _lib.load_library()
    want = expand_rows(*graph, 20)
    total = int(want[0][-1])
    er.same(ctx.graph_expand(graph, 20, max_entries=total), want)
    rc, out = _raw(ctx, graph, 20, max_entries=total - 1)
    assert rc == _lib.FDR_E_ARG and np.array_equal(out, want[0])
    msg = L.fdr_last_error().decode()
    assert "%d entries exceed max_entries = %d" % (total, total - 1) in msg and "indptr_out holds the counts" in msg
    _nothing_held(ctx)
    with pytest.raises(_lib.FedrannHipError, match="exceed max_entries"):
        ctx.graph_expand(graph, 20, max_entries=total - 1)


def test_the_fetch_rules(ctx):
    graph = gr.drawn(65, seed=51)
    L = _lib.load_library()
    ctx.graph_free()
    _nothing_held(ctx)
    rc, out = _raw(ctx, graph, 20, 3, 60)
    total = int(out[-1])
    assert rc == 0 and total > 0
    ix = np.full(total + 1, -7, np.int32)
    for wrong in (total - 1, total + 1, 0):
        assert L.fdr_graph_expand_fetch(ctx._h, wrong, ix.ctypes.data) == _lib.FDR_E_ARG
        assert ("entries = %d, the held result has %d" % (wrong, total)).encode() in L.fdr_last_error()
    assert L.fdr_graph_expand_fetch(ctx._h, total, None) == _lib.FDR_E_ARG
    assert np.all(ix == -7)
    other = gr.drawn(300, seed=52, shuffled=True)
    sym = ctx.graph_symmetrize(other, "union")  # held across a symmetrise call and a components call
    ctx.graph_components(other)
    for _ in range(2):  # (still held; twice is fine)
        assert L.fdr_graph_expand_fetch(ctx._h, total, ix.ctypes.data) == 0
        er.same((out, ix[:total].copy()), expand_rows(*graph, 20, 3, 60))
    assert ix[total] == -7
    same(sym, symmetrize_rows(*other, "union"))
    ctx.graph_free()
    _nothing_held(ctx)
    ctx.graph_free()  # (with nothing to free)
    er.same(ctx.graph_expand(graph, 20), expand_rows(*graph, 20))


def test_the_symmetrised_graph_held_before_the_call_is_still_fetchable(ctx):
    L = _lib.load_library()
    graph, other = gr.drawn(300, seed=61, shuffled=True), gr.drawn(700, seed=62, shuffled=True)
    want = symmetrize_rows(*graph, "mutual")
    ip = np.full(301, -1, np.int64)
    assert L.fdr_graph_symmetrize(ctx._h, 1, 300, graph[0].ctypes.data, graph[1].ctypes.data, graph[2].ctypes.data,
                                  1 << 27, ip.ctypes.data) == 0
    er.same(ctx.graph_expand(other, 128), expand_rows(*other, 128))  # (a larger graph: the shared input arrays regrow)
    total = int(ip[-1])
    idx, dist = np.empty(total, np.int32), np.empty(total, np.float32)
    assert L.fdr_graph_symmetrize_fetch(ctx._h, total, idx.ctypes.data, dist.ctypes.data) == 0
    same((ip, idx, dist), want)


def _edited(graph, fn):
    out = tuple(a.copy() for a in graph)
    fn(*out)
    return out


def _refused(ctx, graph, match, lo=0, hi=None):
    L = _lib.load_library()
    rc, out = _raw(ctx, graph, 5, lo, hi)
    assert rc == _lib.FDR_E_ARG and np.all(out == -7)
    assert re.search(match, L.fdr_last_error().decode()), L.fdr_last_error()
    _nothing_held(ctx)
    with pytest.raises(ValueError, match=match):  # the model names the same row and rule
        expand_rows(*graph, 5, lo, hi)


def test_device_refusals_name_the_smallest_row_and_rule(ctx):
    good = gr.drawn(65, seed=31, shuffled=True, lengths=(5, 63, 64, 65))
    ip = good[0]
    last = int(ip[65] - ip[64]) - 1

    def index(r, j, v):
        return lambda _, ix, ds: ix.__setitem__(int(ip[r]) + j, v)

    def distance(r, j, v):
        return lambda _, ix, ds: ds.__setitem__(int(ip[r]) + j, v)
    for r, j in ((0, 0), (64, last), (30, 4)):
        for lo, hi in ((0, None), (10, 20), (7, 7)):  # the bad row inside the range, outside it, and no range at all
            _refused(ctx, _edited(good, index(r, j, -3)), "row %d: an index outside" % r, lo, hi)
            _refused(ctx, _edited(good, index(r, j, 65)), "row %d: an index outside" % r, lo, hi)
            _refused(ctx, _edited(good, distance(r, j, -0.5)), "row %d: a distance that is negative or NaN" % r, lo, hi)
        _refused(ctx, _edited(good, distance(r, j, np.nan)), "row %d: a distance that is negative or NaN" % r)
        er.same(ctx.graph_expand(good, 5), expand_rows(*good, 5))
    _refused(ctx, _edited(good, distance(3, 1, -0.0)), "row 3: a distance that is negative or NaN")
    several = _edited(_edited(good, distance(5, 1, np.nan)), index(40, 0, -2))
    _refused(ctx, several, "row 5: a distance", 41, 65)  # the smallest (row, rule), outside the rows asked for
    _refused(ctx, _edited(several, index(5, 3, 99)), "row 5: an index outside")
    with pytest.raises(_lib.FedrannHipError, match="row 5: a distance"):
        ctx.graph_expand(several, 5)
    twice = _edited(good, lambda _, ix, ds: ix.__setitem__(int(ip[0]) + 1, ix[int(ip[0])]))
    er.same(ctx.graph_expand(twice, 5), expand_rows(*twice, 5))  # an index listed twice is not refused


def test_the_limits_in_the_library(ctx):
    L = _lib.load_library()
    fn = L.fdr_graph_expand
    ip, ix, ds = gr.drawn(2, seed=61, lengths=(2,))
    out = np.full(3, -7, np.int64)
    p = [a.ctypes.data for a in (ip, ix, ds, out)]
    assert fn(ctx._h, 2, p[0], p[1], p[2], 2, 0, 2, 1 << 20, p[3]) == 0 and out[-1] > 0
    out[:] = -7
    bad = _lib.FDR_E_ARG
    assert fn(ctx._h, 2, None, p[1], p[2], 2, 0, 2, 1 << 20, p[3]) == bad  # null pointers
    assert fn(ctx._h, 2, p[0], None, p[2], 2, 0, 2, 1 << 20, p[3]) == bad
    assert fn(ctx._h, 2, p[0], p[1], None, 2, 0, 2, 1 << 20, p[3]) == bad
    assert fn(ctx._h, 2, p[0], p[1], p[2], 2, 0, 2, 1 << 20, None) == bad
    for fan in (0, -1, 129):
        assert fn(ctx._h, 2, p[0], p[1], p[2], fan, 0, 2, 1 << 20, p[3]) == bad and b"fan=" in L.fdr_last_error()
    for n in (0, -1, 2 ** 31):
        assert fn(ctx._h, n, p[0], p[1], p[2], 2, 0, 0, 1 << 20, p[3]) == bad and b"n (" in L.fdr_last_error()
    for lo, nq in ((-1, 1), (0, 3), (2, 1), (3, 0), (0, -1)):
        assert fn(ctx._h, 2, p[0], p[1], p[2], 2, lo, nq, 1 << 20, p[3]) == bad and b"no range" in L.fdr_last_error()
    for cap in (0, 2 ** 31):
        assert fn(ctx._h, 2, p[0], p[1], p[2], 2, 0, 2, cap, p[3]) == bad and b"max_entries" in L.fdr_last_error()
    for broken in ([0, 3, 2], [1, 2, 4], [0, -1, 4]):
        b = np.array(broken, np.int64)
        assert fn(ctx._h, 2, b.ctypes.data, p[1], p[2], 2, 0, 2, 1 << 20, p[3]) == bad
    big = np.array([0, 2 ** 31], np.int64)
    assert fn(ctx._h, 1, big.ctypes.data, p[1], p[2], 2, 0, 1, 1 << 20, p[3]) == bad and b"2^31" in L.fdr_last_error()
    assert np.all(out == -7)  # no refusal wrote anything
    _nothing_held(ctx)
    assert fn(ctx._h, 2, p[0], p[1], p[2], 2, 1, 0, 1 << 20, p[3]) == 0 and out[0] == 0  # nq == 0: an empty result, held
    assert L.fdr_graph_expand_fetch(ctx._h, 0, None) == 0
