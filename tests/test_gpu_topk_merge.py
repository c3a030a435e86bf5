"""fdr_topk_merge on the GPU against distributed.merge_sparse_topk, bit for bit, on lists where ties decide almost
everything: distances from {0, 0.25, 1} only, distinct indices dealt to the parts at random, every row sorted by key."""
import numpy as np
import pytest

from fedrann_amd import _lib
from fedrann_amd.distributed import merge_sparse_topk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def _keys(idx, dist):
    return (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint32)


def _sorted_rows(idx, dist):
    """[..., kp] rows put in ascending key order."""
    order = np.argsort(_keys(idx, np.ascontiguousarray(dist)), axis=-1, kind="stable")
    return (np.ascontiguousarray(np.take_along_axis(idx, order, axis=-1)),
            np.ascontiguousarray(np.take_along_axis(dist, order, axis=-1)))


def _lists(nq, n_parts, kp, seed, levels=(0.0, 0.25, 1.0)):
    """(idx_parts int32, dist_parts float32) [n_parts, nq, kp]: per query a random permutation of more indices than
    there are slots, dealt to the parts; distances drawn from `levels`; rows sorted by key."""
    rng = np.random.default_rng(seed)
    slots = n_parts * kp
    pool = np.tile(np.arange(slots + 37, dtype=np.int32) * 3 + 1, (nq, 1))
    idx = rng.permuted(pool, axis=1)[:, :slots].reshape(nq, n_parts, kp).transpose(1, 0, 2)
    dist = rng.choice(np.asarray(levels, np.float32), size=(n_parts, nq, kp))
    return _sorted_rows(np.ascontiguousarray(idx), dist)


def _model(idx_parts, dist_parts, k):
    return merge_sparse_topk([(idx_parts[p], dist_parts[p]) for p in range(idx_parts.shape[0])], k)


def _same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("kp", [1, 20, 128])
@pytest.mark.parametrize("n_parts", [1, 2, 3, 64])
@pytest.mark.parametrize("nq", [1, 65, 1000])
def test_merge_is_the_model_bit_for_bit(ctx, nq, n_parts, kp):
    idx_parts, dist_parts = _lists(nq, n_parts, kp, seed=1000 * nq + 10 * n_parts + kp)
    for k in sorted({1, kp, min(128, n_parts * kp)}):  # (kp <= n_parts * kp: all admissible)
        _same(ctx.topk_merge(idx_parts, dist_parts, k), _model(idx_parts, dist_parts, k))


def test_one_part_wins_every_slot(ctx):
    idx_parts, dist_parts = _lists(65, 3, 20, seed=1)
    dist_parts[:] = 1.0
    dist_parts[1] = 0.0
    idx_parts, dist_parts = _sorted_rows(idx_parts, dist_parts)
    got = ctx.topk_merge(idx_parts, dist_parts, 20)
    _same(got, _model(idx_parts, dist_parts, 20))
    _same(got, (idx_parts[1], dist_parts[1]))


@pytest.mark.parametrize("n_parts,kp", [(3, 20), (2, 64), (1, 128), (64, 2), (5, 7)])
def test_every_part_is_exhausted(ctx, n_parts, kp):
    idx_parts, dist_parts = _lists(65, n_parts, kp, seed=2)
    k = n_parts * kp
    got = ctx.topk_merge(idx_parts, dist_parts, k)
    _same(got, _model(idx_parts, dist_parts, k))
    assert np.array_equal(np.sort(got[0], axis=1), np.sort(idx_parts.transpose(1, 0, 2).reshape(65, k), axis=1))


def test_sixty_four_parts_of_one(ctx):
    idx_parts, dist_parts = _lists(65, 64, 1, seed=3)
    for k in (1, 63, 64):
        _same(ctx.topk_merge(idx_parts, dist_parts, k), _model(idx_parts, dist_parts, k))


def test_denormal_and_extreme_distances(ctx):
    tiny = np.array([1], np.uint32).view(np.float32)[0]  # the smallest denormal
    levels = (0.0, tiny, np.float32(1e-40), np.finfo(np.float32).tiny, 1.0, np.float32(3e38), np.inf)
    idx_parts, dist_parts = _lists(65, 3, 20, seed=4, levels=levels)
    assert np.any(dist_parts.view(np.uint32) == 1) and np.any(np.isinf(dist_parts))
    for k in (1, 20, 60):
        _same(ctx.topk_merge(idx_parts, dist_parts, k), _model(idx_parts, dist_parts, k))


def test_the_index_alone_orders_equal_distances(ctx):
    idx_parts, dist_parts = _lists(65, 3, 20, seed=5, levels=(1.0,))
    got = ctx.topk_merge(idx_parts, dist_parts, 20)
    _same(got, _model(idx_parts, dist_parts, 20))
    assert np.all(np.diff(got[0], axis=1) > 0) and np.all(got[1] == 1.0)
    big = idx_parts.copy()
    big[2] = np.iinfo(np.int32).max - np.arange(20, dtype=np.int32)[::-1]  # (the largest indices sort last)
    _same(ctx.topk_merge(big, dist_parts, 60), _model(big, dist_parts, 60))


def test_a_broken_promise_gives_the_duplicate_twice_lower_part_first(ctx):
    idx_parts = np.array([[[4, 9]], [[4, 7]], [[2, 4]]], np.int32)  # index 4 at distance 0.25 in all three parts
    dist_parts = np.array([[[0.25, 0.25]], [[0.25, 1.0]], [[0.0, 0.25]]], np.float32)
    got = ctx.topk_merge(idx_parts, dist_parts, 6)
    _same(got, _model(idx_parts, dist_parts, 6))
    assert got[0].tolist() == [[2, 4, 4, 4, 9, 7]]


def test_no_queries(ctx):
    idx, dist = ctx.topk_merge(np.empty((3, 0, 20), np.int32), np.empty((3, 0, 20), np.float32), 20)
    assert idx.shape == dist.shape == (0, 20)
    L = _lib.load_library()
    assert L.fdr_topk_merge(ctx._h, 0, 3, 20, 20, None, None, None, None) == 0  # FDR_OK without a pointer
    assert L.fdr_topk_merge(ctx._h, 1, 3, 20, 20, None, None, None, None) == -1
    assert L.fdr_topk_merge(ctx._h, 1, 3, 20, 61, None, None, None, None) == -1  # (the limits: in the library too)
    assert L.fdr_topk_merge(ctx._h, 1, 65, 20, 20, None, None, None, None) == -1


def _refused(ctx, idx_parts, dist_parts, k, match):
    nq = idx_parts.shape[1]
    out = np.full((nq, k), -7, np.int32), np.full((nq, k), -7.0, np.float32)
    with pytest.raises(_lib.FedrannHipError, match=match) as e:
        ctx.topk_merge(idx_parts, dist_parts, k, out=out)
    assert "(-1)" in str(e.value)  # FDR_E_ARG
    assert np.all(out[0] == -7) and np.all(out[1] == -7.0)  # nothing was written


def test_refusals_write_nothing_and_the_next_call_is_correct(ctx):
    nq, n_parts, kp, k = 65, 3, 20, 20
    good = _lists(nq, n_parts, kp, seed=6)
    want = _model(*good, k)
    _same(ctx.topk_merge(*good, k), want)

    idx, dist = good[0].copy(), good[1].copy()  # an unsorted row: the last part of the last query
    idx[-1, -1, [3, 4]] = idx[-1, -1, [4, 3]]
    dist[-1, -1, [3, 4]] = dist[-1, -1, [4, 3]]
    _refused(ctx, idx, dist, k, "part 2, query 64: .*ascending")
    _same(ctx.topk_merge(*good, k), want)

    idx = good[0].copy()  # a repeated entry in a row is out of order too
    dist = good[1].copy()
    idx[0, 10, 1], dist[0, 10, 1] = idx[0, 10, 0], dist[0, 10, 0]
    _refused(ctx, idx, dist, k, "part 0, query 10: .*ascending")

    dist = good[1].copy()  # a negative distance (sorted where it stands by value; refused by its sign)
    dist[1, 7, 0] = -0.5
    _refused(ctx, good[0], dist, k, "part 1, query 7: .*negative or NaN")
    dist[1, 7, 0] = -0.0
    _refused(ctx, good[0], dist, k, "part 1, query 7: .*negative or NaN")

    dist = good[1].copy()  # a NaN, at the end of a row where its bits are in order
    dist[2, 0, -1] = np.nan
    _refused(ctx, good[0], dist, k, "part 2, query 0: .*negative or NaN")

    idx = good[0].copy()  # a negative index
    idx[0, 33, 5] = -1
    _refused(ctx, idx, good[1], k, "part 0, query 33: .*negative index")

    idx = good[0].copy()  # two violations: the report is the smallest (query, part)
    idx[2, 5, 0] = -3
    idx[1, 5, 2] = -3
    idx[0, 40, 0] = -3
    _refused(ctx, idx, good[1], k, "part 1, query 5: .*negative index")
    _same(ctx.topk_merge(*good, k), want)


def test_the_sparse_index_and_the_trace_stay_as_they_are(ctx):
    from fedrann_amd.synth import synth
    s = synth(300, seed=9, doubling=True)
    with ctx.sparse_index(s["indptr"], s["indices"], None, s["n_features"], metric="jaccard") as index:
        before = index.search(10, 0, 100)
        trace, info = ctx.last_knn_trace(), index.info()
        lists = _lists(1000, 8, 20, seed=7)
        _same(ctx.topk_merge(*lists, 20), _model(*lists, 20))
        assert ctx.last_knn_trace() == trace and index.info() == info
        _same(index.search(10, 0, 100), before)
