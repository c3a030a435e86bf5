"""Every stage owns its device scratch and its state (one struct each in the context).  The k-mer search, the k-mer
count / merge and the sparse index: a context that has run every stage in turn, every buffer regrown at least once on
the way, gives the bits of a fresh context for every call, and a counting table released by a fetch cannot be resumed.
The dense calls: the result staging that the dense and the sparse searches share, the projection under reloads, and
the capture across calls, each on one context against fresh ones."""
import numpy as np
import pytest

from _kmer_inputs import library_text, random_bases
from _paths_rows import _paths_input
from fedrann_amd import _lib
from fedrann_amd import kmer_search as ks
from fedrann_amd.precompute import build_precompute_matrix
from test_gpu_sparse_knn import _hard_rows

pytestmark = pytest.mark.gpu

K = 7
F = 1 << 25


def _reads(seed, n_reads, mean_len):
    """n_reads pieces of a random genome (a few N and lower-case characters; lengths 0 and below K among them)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 2 * mean_len, size=n_reads)
    genome = random_bases(rng, 4 * mean_len)
    pieces = []
    for n in lens:
        a = int(rng.integers(0, len(genome) - n))
        r = bytearray(genome[a:a + n])
        for p in np.flatnonzero(rng.random(int(n)) < 0.01):
            r[p] = ord("N") if p % 2 else r[p] | 0x20
        pieces.append(bytes(r))
    off = np.zeros(n_reads + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    return np.frombuffer(b"".join(pieces), dtype=np.uint8), off


def _library(seed, n):
    rng = np.random.default_rng(seed)
    fwd = list({random_bases(rng, K) for _ in range(n)})
    return ks.load_kmer_library(library_text(rng, fwd, K, junk=False), K)


def _runs(seed, n_runs, per_run):
    """n_runs ascending runs of unique codes that overlap heavily, with counts 1 .. 3."""
    rng = np.random.default_rng(seed)
    runs = [np.unique(rng.integers(0, 4 * per_run, size=per_run, dtype=np.uint64)) for _ in range(n_runs)]
    run_off = np.zeros(n_runs + 1, dtype=np.int64)
    run_off[1:] = np.cumsum([r.size for r in runs])
    return run_off, np.concatenate(runs), rng.integers(1, 4, size=int(run_off[-1])).astype(np.uint64)


def _inputs():
    small, large = _reads(1, 200, 300), _reads(2, 500, 400)  # (the second search is the larger one)
    sp_small, sp_large = _hard_rows(120, seed=3, n_ids=200)[:3], _hard_rows(300, seed=4, n_ids=300)[:3]
    assert np.any(np.diff(sp_large[0]) == 0)  # (zero rows)
    return dict(small=small, large=large, lib_small=_library(5, 150), lib_large=_library(6, 400),
                sp_small=sp_small, sp_large=sp_large, runs=_runs(7, 3, 20_000))


def _search(c, inp, reads, lib):
    return c.kmer_search(inp[reads][0], inp[reads][1], inp[lib], K)


def _count(c, inp):
    """The small reads counted in blocks of a fifth of their characters; the block setting back at 0 afterwards."""
    seqs, off = inp["small"]
    try:
        c.set_kmer_count_block(int(off[-1]) // 5)
        got = c.kmer_count(seqs, off, K, 2)
        assert c.last_kmer_count_blocks() >= 3
    finally:
        c.set_kmer_count_block(0)
    return got


def _sparse(c, inp, rows, metric):
    """(The index is not closed: the next build replaces it and grows its buffers.)"""
    indptr, indices, values = inp[rows]
    return c.sparse_index(indptr, indices, values if metric == "cosine" else None, F, metric=metric).search(5)


def _merge(c, inp):
    return c.kmer_count_merge(*inp["runs"], 2)


STAGES = [
    ("search, small", lambda c, i: _search(c, i, "small", "lib_small")),
    ("search, large", lambda c, i: _search(c, i, "large", "lib_large")),
    ("count in blocks", _count),
    ("sparse index, small, cosine", lambda c, i: _sparse(c, i, "sp_small", "cosine")),
    ("sparse index, small, jaccard", lambda c, i: _sparse(c, i, "sp_small", "jaccard")),
    ("sparse index, large, cosine", lambda c, i: _sparse(c, i, "sp_large", "cosine")),
    ("sparse index, large, jaccard", lambda c, i: _sparse(c, i, "sp_large", "jaccard")),
    ("merge of three runs", _merge),  # (60 000 entries: more than the count's table of at most 4^7 / 2 codes)
    ("search, small, again", lambda c, i: _search(c, i, "small", "lib_small")),
]


def _same_bits(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), what


def test_one_context_runs_every_stage_in_turn():
    inp = _inputs()
    with _lib.Context(0) as one:
        got = [stage(one, inp) for _, stage in STAGES]
    for (what, stage), g in zip(STAGES, got):
        with _lib.Context(0) as fresh:
            _same_bits(g, stage(fresh, inp), what)
    assert got[0][1].size > 0 and got[1][1].size > got[0][1].size  # the searches hit, the second one more
    assert got[2][0].size > 0 and got[7][0].size > got[2][0].size  # k-mers kept; the merge keeps more than the count
    # the merge against numpy: the summed counts of the runs' codes, thresholded
    run_off, codes, counts = inp["runs"]
    u, inv = np.unique(codes, return_inverse=True)
    tot = np.bincount(inv, weights=counts.astype(np.float64)).astype(np.uint64)
    assert np.array_equal(got[7][0], u[tot >= 2]) and np.array_equal(got[7][1], tot[tot >= 2])


def test_a_released_count_cannot_be_resumed():
    """begin, add, then a search whose fetch releases all k-mer scratch, the accumulated table included: the next add
    is refused before any GPU work (the count's state is released with its table); a new count is as in one piece."""
    seqs, off = _reads(1, 200, 300)
    lib = _library(5, 150)
    half = 100
    with _lib.Context(0) as c:
        want = c.kmer_count(seqs, off, K, 2)
        c.kmer_count_begin(K)
        c.kmer_count_add(seqs[:off[half]], off[:half + 1])
        c.kmer_search(seqs, off, lib, K)
        with pytest.raises(_lib.FedrannHipError, match="begin first"):
            c.kmer_count_add(seqs[off[half]:], off[half:] - off[half])
        c.kmer_count_begin(K)
        c.kmer_count_add(seqs[:off[half]], off[:half + 1])
        c.kmer_count_add(seqs[off[half]:], off[half:] - off[half])
        _same_bits(c.kmer_count_finish(2), want, "count after a refused add")
    assert want[0].size > 0


def _fresh(call):
    with _lib.Context(0) as c:
        return call(c)


def test_result_staging_serves_dense_and_sparse_searches_in_turn():
    """knn (300 x 5 results) -> a sparse search (2000 x 20: the staging grows under the sparse index's hands) -> the
    same knn (in the larger staging) -> a search of 40 rows with k = 3 (likewise): each as on a fresh context."""
    E = np.random.default_rng(11).standard_normal((300, 32)).astype(np.float32)
    indptr, indices, values = _hard_rows(2000, seed=12, n_ids=400)[:3]

    def index(c):
        return c.sparse_index(indptr, indices, values, F)

    with _lib.Context(0) as one:
        first = one.knn(E, 5)
        sp = index(one)
        wide = sp.search(20)
        again = one.knn(E, 5)
        narrow = sp.search(3, 100, 140)
    assert wide[0].shape == (2000, 20) and narrow[0].shape == (40, 3)
    _same_bits(first, _fresh(lambda c: c.knn(E, 5)), "knn")
    _same_bits(again, first, "knn after the sparse search")
    _same_bits(wide, _fresh(lambda c: index(c).search(20)), "sparse search")
    _same_bits(narrow, _fresh(lambda c: index(c).search(3, 100, 140)), "sparse search of a row range")


def _projection_and_rows(n_features, d, n_rows, ids_per_row, seed):
    """(P, indptr, indices): a projection over n_features, and rows of about ids_per_row ascending distinct ids."""
    rng = np.random.default_rng(seed)
    P = build_precompute_matrix(rng.integers(1, 50, size=n_features // 2), d)
    ids = np.sort(rng.integers(0, n_features, size=(n_rows, ids_per_row), dtype=np.int32), axis=1)
    keep = np.ones(ids.shape, dtype=bool)
    keep[:, 1:] = ids[:, 1:] != ids[:, :-1]
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(keep.sum(axis=1))
    return P, indptr, np.ascontiguousarray(ids[keep])


def test_projection_reloads():
    """1 000 features at d = 16, then 50 000 at d = 64 (every table regrows; 1.1 M ids: the pipelined upload, every
    array of which grows as well), then the first again, in the larger tables: each embed as on a fresh context.  No
    projection: the state error."""
    small = _projection_and_rows(1_000, 16, 200, 30, seed=21)
    large = _projection_and_rows(50_000, 64, 6_000, 190, seed=22)
    assert large[1][-1] > 1 << 20 > small[1][-1]

    def embed(c, P, indptr, indices):
        c.projection_load(P.indptr, P.indices, P.data, P.shape[0], P.shape[1])
        return c.embed(indptr, indices)

    with _lib.Context(0) as one:
        with pytest.raises(_lib.FedrannHipError, match="no projection loaded"):
            one.embed(small[1], small[2])
        got = [embed(one, *p) for p in (small, large, small)]
    for g, p, what in zip(got, (small, large, small), ("small", "large", "small again")):
        assert g.shape == (p[1].size - 1, p[0].shape[1]) and np.any(g != 0), what
        _same_bits([g], [_fresh(lambda c: embed(c, *p))], what)


def _captured_call(c, E, k):
    """A prefilter-mode knn of E with candidate and range capture on, duplicate-row classes off: (idx, dist, keys,
    range sets).  The range sets in a canonical form: the pass appends queries, and a query's rows, in the order its
    atomics fall, so queries are sorted and so are the rows of each (none overflows RANGE_CAP here: every set is whole)."""
    idx, dist = c.knn(E, k)
    tr = c.last_knn_trace()
    assert tr["kind"] == "prefilter" and tr["range_queries"] > 0, tr
    keys, qbits = c.last_candidates(E.shape[0], tr["kp"])
    rq, theta, cnt, rows = c.last_range_sets(tr["range_queries"])
    assert 0 < cnt.max() <= _lib.RANGE_CAP
    order = np.argsort(rq, kind="stable")
    return idx, dist, keys, np.array([qbits], np.int32), rq[order], theta[order], cnt[order], np.sort(rows[order], axis=1)


def test_capture_across_calls():
    """A captured 9 000-row prefilter call with a range pass, a 300-row exact call (the getters refuse, the arrays
    stay), the first call again: the same keys and sets, which are a fresh context's too."""
    E = _paths_input(9_000, 100, seed=31, plateau=(12, 150), overflow=0).cpu().numpy()
    few = np.random.default_rng(32).standard_normal((300, 100)).astype(np.float32)

    def setup(c):
        c.set_dedup_mode("off")
        c.set_knn_capture(_lib.CAPTURE_CANDIDATES | _lib.CAPTURE_RANGE)
        c.set_knn_mode("prefilter")

    with _lib.Context(0) as one:
        setup(one)
        first = _captured_call(one, E, 20)
        one.set_knn_mode("exact")
        one.knn(few, 10)
        assert one.last_knn_trace()["kind"] == "exact"
        with pytest.raises(_lib.FedrannHipError, match="last_candidates: the last k-NN call captured no candidates"):
            one.last_candidates(300, 22)
        with pytest.raises(_lib.FedrannHipError, match="last_range_sets: the last k-NN call captured no range pass"):
            one.last_range_sets(1)
        one.set_knn_mode("prefilter")
        second = _captured_call(one, E, 20)
    _same_bits(second, first, "the captured call again")

    def fresh(c):
        setup(c)
        return _captured_call(c, E, 20)

    _same_bits(first, _fresh(fresh), "the captured call on a fresh context")
