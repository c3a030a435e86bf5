"""fdr_radius_merge on the GPU against distributed.merge_sparse_radius, bit for bit, on ragged rows where the index
decides most positions: distances from {0, 0.25, 0.5} only, distinct indices dealt to the parts at random, row lengths
from {0, 0, 1, 63, 64, 65, 300} per (part, query), every row sorted by key."""
import re

import numpy as np
import pytest

from _radius_model import same
from fedrann_amd import _lib
from fedrann_amd.distributed import merge_sparse_radius

pytestmark = pytest.mark.gpu

LENGTHS = (0, 0, 1, 63, 64, 65, 300)
LEVELS = (0.0, 0.25, 0.5)


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def _ragged(lens, seed, levels=LEVELS):
    """lens int [n_parts, nq] -> n_parts parts (indptr, idx, dist): per query a random permutation of more indices than
    its entries, dealt to the parts; distances drawn from `levels`; every row sorted by key."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    n_parts, nq = lens.shape
    idx = [[None] * nq for _ in range(n_parts)]
    dist = [[None] * nq for _ in range(n_parts)]
    for q in range(nq):
        pool = rng.permutation(int(lens[:, q].sum()) + 37).astype(np.int32) * 3 + 1
        at = 0
        for p in range(n_parts):
            i = pool[at:at + lens[p, q]]
            at += int(lens[p, q])
            d = rng.choice(np.asarray(levels, np.float32), size=i.size)
            order = np.lexsort((i, d.view(np.uint32)))
            idx[p][q], dist[p][q] = i[order], d[order]
    parts = []
    for p in range(n_parts):
        ip = np.zeros(nq + 1, np.int64)
        np.cumsum(lens[p], out=ip[1:])
        parts.append((ip, np.concatenate(idx[p]).astype(np.int32) if nq else np.zeros(0, np.int32),
                      np.concatenate(dist[p]).astype(np.float32) if nq else np.zeros(0, np.float32)))
    return parts


def _drawn(nq, n_parts, seed):
    lens = np.random.default_rng(seed).choice(np.asarray(LENGTHS), size=(n_parts, nq))
    return _ragged(lens, seed + 1)


@pytest.mark.parametrize("n_parts", [1, 2, 3, 64])
@pytest.mark.parametrize("nq", [1, 65, 1000])
def test_merge_is_the_model_bit_for_bit(ctx, nq, n_parts):
    parts = _drawn(nq, n_parts, seed=1000 * nq + n_parts)
    got = ctx.radius_merge(parts)
    same(got, merge_sparse_radius(parts))
    assert int(got[0][-1]) == sum(int(p[0][-1]) for p in parts)


def test_one_query_of_5000_entries_over_three_parts(ctx):
    parts = _ragged([[1700], [2500], [800]], seed=2)
    got = ctx.radius_merge(parts)
    same(got, merge_sparse_radius(parts))
    assert got[0].tolist() == [0, 5000]
    key = (got[2].view(np.uint32).astype(np.uint64) << np.uint64(32)) | got[1].astype(np.uint32)
    assert np.all(np.diff(key.astype(np.int64)) > 0)  # (distinct indices: strictly ascending)


def test_one_part_holds_everything(ctx):
    lens = np.zeros((3, 65), np.int64)
    lens[1] = np.random.default_rng(3).choice(np.asarray(LENGTHS), size=65)
    parts = _ragged(lens, seed=3)
    got = ctx.radius_merge(parts)
    same(got, merge_sparse_radius(parts))
    same(got, parts[1])


def test_every_part_is_empty(ctx):
    parts = _ragged(np.zeros((3, 65), np.int64), seed=4)
    got = ctx.radius_merge(parts)
    assert got[0].tolist() == [0] * 66 and got[1].size == got[2].size == 0
    same(got, merge_sparse_radius(parts))
    L = _lib.load_library()
    ips = np.zeros((3, 66), np.int64)
    out = np.full(66, -7, np.int64)
    assert L.fdr_radius_merge(ctx._h, 65, 3, ips.ctypes.data, None, None, out.ctypes.data, None, None) == 0
    assert np.all(out == 0)  # FDR_OK without an entry pointer: the indptr alone is written


def test_no_queries_and_the_limits_in_the_library(ctx):
    z = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    got = ctx.radius_merge([z, z, z])
    assert got[0].tolist() == [0] and got[1].size == 0
    L = _lib.load_library()
    ips = np.zeros((3, 1), np.int64)
    out = np.full(1, -7, np.int64)
    assert L.fdr_radius_merge(ctx._h, 0, 3, ips.ctypes.data, None, None, out.ctypes.data, None, None) == 0
    assert out[0] == 0
    out[:] = -7
    one = np.array([[0, 1]], np.int64)
    o2 = np.full(2, -7, np.int64)
    assert L.fdr_radius_merge(ctx._h, 1, 1, one.ctypes.data, None, None, o2.ctypes.data, None, None) == -1  # null entries
    assert L.fdr_radius_merge(ctx._h, 0, 0, ips.ctypes.data, None, None, out.ctypes.data, None, None) == -1
    assert L.fdr_radius_merge(ctx._h, 0, 65, ips.ctypes.data, None, None, out.ctypes.data, None, None) == -1
    assert L.fdr_radius_merge(ctx._h, -1, 1, ips.ctypes.data, None, None, out.ctypes.data, None, None) == -1
    assert L.fdr_radius_merge(ctx._h, 0, 1, None, None, None, out.ctypes.data, None, None) == -1
    assert L.fdr_radius_merge(ctx._h, 0, 1, ips.ctypes.data, None, None, None, None, None) == -1
    e = np.zeros(4, np.int32)
    for bad in ([[1, 2]], [[0, -1]]):  # (the indptr checks: in the library too)
        b = np.array(bad, np.int64)
        assert L.fdr_radius_merge(ctx._h, 1, 1, b.ctypes.data, e.ctypes.data, e.ctypes.data, o2.ctypes.data,
                                  e.ctypes.data, e.ctypes.data) == -1
    big = np.array([[0, 2 ** 30], [0, 2 ** 30]], np.int64)  # 2^31 entries in all: refused before anything is read
    assert L.fdr_radius_merge(ctx._h, 1, 2, big.ctypes.data, e.ctypes.data, e.ctypes.data, o2.ctypes.data,
                              e.ctypes.data, e.ctypes.data) == -1
    assert b"2^31" in L.fdr_last_error()
    assert out[0] == -7 and np.all(o2 == -7) and np.all(e == 0)  # no refusal wrote anything


def test_pieces_give_the_same_result_and_one_row_above_the_cap_is_refused(ctx, monkeypatch):
    parts = _drawn(65, 3, seed=7)
    want = merge_sparse_radius(parts)
    counts = np.diff(want[0])
    fullest = int(counts.max())
    calls = []
    real = ctx._L.fdr_radius_merge

    class Counting:
        def __getattr__(self, name):
            return getattr(ctx_L, name)

        def fdr_radius_merge(self, *a):
            calls.append(int(a[1]))
            return real(*a)
    ctx_L = ctx._L
    monkeypatch.setattr(ctx, "_L", Counting())
    same(ctx.radius_merge(parts, max_entries=fullest), want)
    assert len(calls) >= 3 and sum(calls) == 65  # (consecutive pieces that tile the queries)
    assert len(calls) == len(_lib.radius_pieces(counts, fullest))
    del calls[:]
    same(ctx.radius_merge(parts, max_entries=int(want[0][-1])), want)
    assert calls == [65]
    with pytest.raises(ValueError, match="query %d alone has %d entries" % (int(np.argmax(counts)), fullest)):
        ctx.radius_merge(parts, max_entries=fullest - 1)


def test_a_broken_promise_gives_the_duplicate_twice_lower_part_first(ctx):
    def part(*rows):
        ip = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=ip[1:])
        flat = [e for r in rows for e in r]
        return ip, np.array([e[0] for e in flat], np.int32), np.array([e[1] for e in flat], np.float32)
    parts = [part([(4, 0.25), (9, 0.25)]), part([(4, 0.25), (7, 0.5)]), part([(2, 0.0), (4, 0.25)])]
    got = ctx.radius_merge(parts)
    same(got, merge_sparse_radius(parts))
    assert got[1].tolist() == [2, 4, 4, 4, 9, 7]
    both = [part([(4, 0.25)]), part([(4, 0.25)])]  # (equal keys alone: two slots, none written twice or left out)
    got = ctx.radius_merge(both)
    assert got[0].tolist() == [0, 2] and got[1].tolist() == [4, 4] and got[2].tolist() == [0.25, 0.25]


def _refused(ctx, parts, match):
    """The raw call on prefilled out arrays: FDR_E_ARG, the message, nothing written."""
    L = _lib.load_library()
    nq = parts[0][0].size - 1
    total = sum(int(p[0][-1]) for p in parts)
    ips = np.stack([p[0] for p in parts])
    ix, ds = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    out = np.full(nq + 1, -7, np.int64), np.full(total, -7, np.int32), np.full(total, -7.0, np.float32)
    rc = L.fdr_radius_merge(ctx._h, nq, len(parts), ips.ctypes.data, ix.ctypes.data, ds.ctypes.data, out[0].ctypes.data,
                            out[1].ctypes.data, out[2].ctypes.data)
    assert rc == -1  # FDR_E_ARG
    assert re.search(match, L.fdr_last_error().decode()), L.fdr_last_error()
    assert np.all(out[0] == -7) and np.all(out[1] == -7) and np.all(out[2] == -7.0)  # nothing was written
    with pytest.raises(_lib.FedrannHipError, match=match):
        ctx.radius_merge(parts)


def _edited(parts, p, fn):
    out = [(a.copy(), b.copy(), c.copy()) for a, b, c in parts]
    fn(*out[p])
    return out


def test_refusals_write_nothing_and_the_next_call_is_correct(ctx):
    lens = np.random.default_rng(8).choice(np.asarray([5, 63, 64, 65, 300]), size=(3, 65))
    lens[1, 20] = 300
    good = _ragged(lens, seed=8)
    want = merge_sparse_radius(good)
    same(ctx.radius_merge(good), want)

    def swap(q, j):  # entries j and j + 1 of row q change places: distinct keys, so the row is out of order
        def fn(ip, ix, ds):
            a = int(ip[q]) + j
            ix[[a, a + 1]], ds[[a, a + 1]] = ix[[a + 1, a]], ds[[a + 1, a]]
        return fn
    _refused(ctx, _edited(good, 2, swap(64, 3)), "part 2, query 64: .*ascending")  # the last part of the last query
    same(ctx.radius_merge(good), want)
    _refused(ctx, _edited(good, 1, swap(20, 255)), "part 1, query 20: .*ascending")  # across two strides of the wave
    _refused(ctx, _edited(good, 1, swap(20, 200)), "part 1, query 20: .*ascending")

    def repeat(ip, ix, ds):  # a repeated entry in a row is out of order too
        a = int(ip[10])
        ix[a + 1], ds[a + 1] = ix[a], ds[a]
    _refused(ctx, _edited(good, 0, repeat), "part 0, query 10: .*ascending")

    def distance(q, j, v):
        def fn(ip, ix, ds):
            ds[int(ip[q]) + j] = v
        return fn
    _refused(ctx, _edited(good, 1, distance(7, 0, -0.5)), "part 1, query 7: .*negative or NaN")
    _refused(ctx, _edited(good, 1, distance(7, 0, -0.0)), "part 1, query 7: .*negative or NaN")
    # NaN distance bits, at the end of a row where they are in order
    _refused(ctx, _edited(good, 2, distance(0, int(lens[2, 0]) - 1, np.nan)), "part 2, query 0: .*negative or NaN")

    def neg_index(q, j):
        def fn(ip, ix, ds):
            ix[int(ip[q]) + j] = -3
        return fn
    _refused(ctx, _edited(good, 0, neg_index(33, 4)), "part 0, query 33: .*negative index")
    two = _edited(_edited(_edited(good, 2, neg_index(5, 0)), 1, neg_index(5, 2)), 0, neg_index(40, 0))
    _refused(ctx, two, "part 1, query 5: .*negative index")  # several violations: the smallest (query, part)
    same(ctx.radius_merge(good), want)


def test_the_sparse_index_its_held_result_and_the_trace_stay_as_they_are(ctx):
    from fedrann_amd.synth import synth
    s = synth(300, seed=9, doubling=True)
    L = _lib.load_library()
    with ctx.sparse_index(s["indptr"], s["indices"], None, s["n_features"], metric="jaccard") as index:
        parts = _drawn(65, 3, seed=11)
        same(ctx.radius_merge(parts), merge_sparse_radius(parts))  # a call before ...
        before = index.radius_search(0.9, 0, 100)
        knn = index.search(10, 0, 100)
        # a radius call whose result is still held by the context: counts taken, hits not yet fetched
        ip = np.full(101, -1, np.int64)
        assert L.fdr_sparse_index_radius_search(ctx._h, np.float32(0.9), 0, 100, 1 << 26, ip.ctypes.data) == 0
        assert np.array_equal(ip, before[0])
        trace, info = ctx.last_knn_trace(), index.info()  # (the radius call's own record)
        same(ctx.radius_merge(parts), merge_sparse_radius(parts))  # ... one between the search and its fetch ...
        total = int(ip[-1])
        idx, dist = np.empty(total, np.int32), np.empty(total, np.float32)
        assert L.fdr_sparse_index_radius_fetch(ctx._h, total, idx.ctypes.data, dist.ctypes.data) == 0
        same((ip, idx, dist), before)
        assert ctx.last_knn_trace() == trace and index.info() == info
        same(ctx.radius_merge(parts), merge_sparse_radius(parts))  # ... and one after
        same(index.radius_search(0.9, 0, 100), before)
        got = index.search(10, 0, 100)
        assert np.array_equal(got[0], knn[0]) and np.array_equal(got[1].view(np.uint32), knn[1].view(np.uint32))
