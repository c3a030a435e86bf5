"""fdr_kmer_count* (GPU) against two witnesses that share nothing with each other: the string model of
_kmer_count_model and the oracle's numpy restatement.  The inputs put read boundaries, invalid bytes and strands at the
places kc_codes_kernel's walk treats specially (chunk staging with 32 bytes of history, the gallop to a thread's first
read, 16-position stretches, the primed / run state, the reverse-complement register), carry them into the later trips
of its grid-stride loop, and drive the all-ones "no k-mer here" marker through the block accumulate, the export and the
threshold.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import _kmer_count_model as M
from _kmer_inputs import random_bases, revcomp
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

BUILDERS = ("boundary_reads", "placed_invalids", "byte_values", "strands_and_palindromes")
STATE = r"\(-5\)"  # FDR_E_STATE


@functools.lru_cache(maxsize=None)
def _case(name, k):
    """(seqs, seq_off, reads, the string model's table at min_count = 1) of one builder."""
    if name == "boundary_reads":
        seqs, off, _ = M.boundary_reads(np.random.default_rng(40 + k), k)
    elif name == "placed_invalids":
        seqs, off, _ = M.placed_invalids(k)
    elif name == "byte_values":
        seqs, off, _ = M.byte_values()
    elif name == "strands_and_palindromes":
        seqs, off, _ = M.strands_and_palindromes(np.random.default_rng(60 + k), k)
    else:
        seqs, off = M.grid_stride_base(k)
    reads = M.to_reads(seqs, off)
    return seqs, off, reads, M.string_count(reads, k, 1)


def _same(got, want, what=""):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64
    assert np.array_equal(got[0], want[0]), "codes differ %s" % (what,)
    assert np.array_equal(got[1], want[1]), "counts differ %s" % (what,)


def _split(seqs, off, c):
    return (seqs[:off[c]], off[:c + 1]), (seqs[off[c]:], off[c:] - off[c])


@pytest.mark.parametrize("k", M.KS)
def test_count_at_the_edges_equals_both_witnesses(ctx, oracle, k):
    for name in BUILDERS:
        seqs, off, reads, table = _case(name, k)
        assert table[0].size > 0 and seqs.size < 100_000
        for min_count in (1, 2):
            got = ctx.kmer_count(seqs, off, k, min_count)
            _same(got, M.threshold(table, min_count), (name, k, min_count, "string model"))
            _same(got, oracle.kmer_count(reads, k, min_count), (name, k, min_count, "oracle"))
        above = int(table[1].max()) + 1
        none = ctx.kmer_count(seqs, off, k, above)
        assert none[0].size == 0 and none[1].size == 0
        _same(ctx.kmer_count(seqs, off, k, above - 1), M.threshold(table, above - 1), (name, k, "after nothing kept"))


def _grid_stride_need(ctx):
    """More characters than one trip of the grid-stride loops of kc_codes_kernel / ks_search_kernel covers:
    min(chunks, CUs * 8) workgroups of 4096 characters, and three chunks more."""
    cus = ctx.device_info()["cus"]
    assert cus > 0
    return cus * 8 * M.CHUNK + 3 * M.CHUNK


@pytest.mark.parametrize("k", [15, 31])
def test_count_beyond_one_trip_of_the_grid_stride_loop(ctx, oracle, k):
    """boundary_reads + placed_invalids tiled until some workgroup takes a second chunk (and, the base's total being
    odd, every copy lies differently in the chunks), with one more read behind.  Expected: the base's table times the
    number of copies, merged with the tail's."""
    need = _grid_stride_need(ctx)
    base_seqs, base_off, base_reads, base = _case("grid_stride_base", k)
    _same(oracle.kmer_count(base_reads, k, 1), base, "oracle on the base")
    times = M.times_to_exceed(int(base_off[-1]), need)
    seqs, off, e = M.tiled(base_seqs, base_off, times)
    tail = random_bases(np.random.default_rng(3), 150) + b"N" + random_bases(np.random.default_rng(4), 151)
    seqs = np.concatenate([seqs, np.frombuffer(tail, dtype=np.uint8)])
    off = np.concatenate([off, [off[-1] + len(tail)]])
    total = int(off[-1])
    print("grid-stride count: k = %d, %d CUs, %d copies of %d characters + %d = %d characters (> %d)"
          % (k, ctx.device_info()["cus"], times, e["base_total"], len(tail), total, need))
    assert total > need and total == seqs.size and e["copy_shifts"] == min(16, times)
    want = M.merge_tables(M.scale_table(base, times), M.string_count([tail], k, 1))
    try:
        ctx.set_kmer_count_block(0)
        _same(ctx.kmer_count(seqs, off, k, 1), want, "one block")
        assert ctx.last_kmer_count_blocks() == 1
        ctx.set_kmer_count_block(total // 3 + 1)
        _same(ctx.kmer_count(seqs, off, k, 1), want, "blocks")
        assert ctx.last_kmer_count_blocks() in (3, 4)
        _same(ctx.kmer_count(seqs, off, k, times + 1), M.threshold(want, times + 1), "blocks, thresholded")
    finally:
        ctx.set_kmer_count_block(0)


# ---- blocks and the marker -----------------------------------------------------------------------------------------
BLOCK = 192  # characters of every block below: set_kmer_count_block(BLOCK + 1) cuts the read set exactly there


def _block(rng, k, kind, genome):
    """Reads of one block: 'R' pieces of the genome (both strands), 'N' only invalid bytes, 'S' only reads shorter
    than k."""
    if kind == "R":
        out = []
        for _ in range(3):
            a = int(rng.integers(0, len(genome) - 64))
            out.append(revcomp(genome[a:a + 64]) if rng.random() < 0.4 else genome[a:a + 64])
        return out
    if kind == "N":
        return [b"N" * 64, b"-" * 64, b"\xff" * 64]
    assert kind == "S" and k >= 2
    lens = [k - 1] * (BLOCK // (k - 1)) + [BLOCK % (k - 1)]
    return [random_bases(rng, n) for n in lens]


def _blocks(rng, k, layout):
    genome = random_bases(rng, 400)  # (short: the blocks share k-mers, so the accumulate sums)
    reads = []
    for kind in layout:
        b = _block(rng, k, kind, genome)
        assert sum(len(r) for r in b) == BLOCK
        reads += b
    return reads


@pytest.mark.parametrize("k", [2, 16, 31])
def test_a_block_that_leaves_only_the_marker(ctx, oracle, k):
    rng = np.random.default_rng(200 + k)
    try:
        for layout in ("NRRR", "RRNR", "RRRN", "SRRR", "RSRR", "RRRS", "NRSRN", "SNRRR"):
            reads = _blocks(rng, k, layout)
            seqs, off = M.from_reads(reads)
            want = M.string_count(reads, k, 1)
            _same(oracle.kmer_count(reads, k, 1), want, (layout, "oracle"))
            assert want[0].size > 0 and int(want[1].max()) > 1
            for min_count in (1, 2):
                ctx.set_kmer_count_block(0)
                _same(ctx.kmer_count(seqs, off, k, min_count), M.threshold(want, min_count), (layout, "one piece"))
                assert ctx.last_kmer_count_blocks() == 1
                ctx.set_kmer_count_block(BLOCK + 1)
                _same(ctx.kmer_count(seqs, off, k, min_count), M.threshold(want, min_count), (layout, "blocks"))
                assert ctx.last_kmer_count_blocks() == len(layout)
    finally:
        ctx.set_kmer_count_block(0)


@pytest.mark.parametrize("k", [2, 16, 31])
def test_a_table_that_is_only_the_marker(ctx, k):
    rng = np.random.default_rng(300 + k)
    reads = _blocks(rng, k, "NSN")
    seqs, off = M.from_reads(reads)
    assert M.string_count(reads, k, 1)[0].size == 0
    try:
        for block, n_blocks in ((0, 1), (BLOCK + 1, 3)):
            ctx.set_kmer_count_block(block)
            codes, counts = ctx.kmer_count(seqs, off, k, 1)
            assert codes.size == 0 and counts.size == 0 and codes.dtype == np.uint64
            assert ctx.last_kmer_count_blocks() == n_blocks
            ctx.kmer_count_begin(k)
            ctx.kmer_count_add(seqs, off)
            assert ctx.kmer_count_export_dev(0, 1).tolist() == [0, 0]
            assert ctx.last_kmer_count_blocks() == n_blocks  # (the blocks that produced runs: here the marker's)
            codes, counts = ctx.kmer_count_finish(1)
            assert codes.size == 0 and counts.size == 0
    finally:
        ctx.set_kmer_count_block(0)
    # the context counts on
    real = _blocks(rng, k, "RR")
    s2, o2 = M.from_reads(real)
    _same(ctx.kmer_count(s2, o2, k, 1), M.string_count(real, k, 1))


@pytest.mark.parametrize("k", [16, 31])
def test_the_threshold_applies_to_totals_over_blocks(ctx, k):
    """A k-mer seen once in each of three blocks (in one of them reverse-complemented) passes min_count = 3 and
    fails min_count = 4."""
    rng = np.random.default_rng(400 + k)
    x = random_bases(rng, k)
    assert x != revcomp(x)
    reads = []
    for b in range(3):
        w = revcomp(x) if b == 1 else x
        a = int(rng.integers(0, 64 - k))
        reads += [b"N" * a + w + b"N" * (64 - k - a), random_bases(rng, 64), random_bases(rng, 64)]
    seqs, off = M.from_reads(reads)
    table = M.string_count(reads, k, 1)
    code = M.string_count([x], k, 1)[0]
    assert table[1][table[0] == code[0]].tolist() == [3] and int(table[1].max()) == 3
    try:
        ctx.set_kmer_count_block(BLOCK + 1)
        got = ctx.kmer_count(seqs, off, k, 3)
        assert ctx.last_kmer_count_blocks() == 3
        _same(got, (code, np.array([3], dtype=np.uint64)))
        got = ctx.kmer_count(seqs, off, k, 4)
        assert got[0].size == 0 and got[1].size == 0
        _same(ctx.kmer_count(seqs, off, k, 1), table)
    finally:
        ctx.set_kmer_count_block(0)


def test_empty_reads_at_block_edges_change_nothing(ctx):
    k = 16
    rng = np.random.default_rng(500)
    real = _blocks(rng, k, "RRRR")
    want = M.string_count(real, k, 1)
    with_empties = [b""] * 3
    for i in range(0, len(real), 3):
        with_empties += real[i:i + 3] + [b""] * 3  # (between the blocks and at the very end)
    seqs, off = M.from_reads(with_empties)
    empties = (np.zeros(0, dtype=np.uint8), np.zeros(5, dtype=np.int64))
    nothing = (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    try:
        for block, n_blocks in ((0, 1), (BLOCK + 1, 4)):
            ctx.set_kmer_count_block(block)
            _same(ctx.kmer_count(seqs, off, k, 1), want, "empty reads inside")
            assert ctx.last_kmer_count_blocks() == n_blocks
            # pieces made only of empty reads, and of no reads, first, between and last
            ctx.kmer_count_begin(k)
            ctx.kmer_count_add(*empties)
            ctx.kmer_count_add(*nothing)
            assert ctx.last_kmer_count_blocks() == 0 and ctx.kmer_count_export_dev(0, 1).tolist() == [0, 0]
            a, b = _split(*M.from_reads(real), 6)
            ctx.kmer_count_add(*a)
            ctx.kmer_count_add(*empties)
            ctx.kmer_count_add(*nothing)
            ctx.kmer_count_add(*b)
            ctx.kmer_count_add(*empties)
            assert ctx.last_kmer_count_blocks() == (2 if block == 0 else 4)
            _same(ctx.kmer_count_finish(1), want, "pieces of empty reads")
    finally:
        ctx.set_kmer_count_block(0)


# ---- streaming -----------------------------------------------------------------------------------------------------
def test_streamed_pieces_cut_at_empty_and_short_reads(ctx):
    k = 15
    seqs, off, reads, table = _case("boundary_reads", k)
    lens = np.diff(off)
    inner = np.arange(10, lens.size - 10)
    empty = int(inner[lens[inner] == 0][20])
    short = int(inner[(lens[inner] > 0) & (lens[inner] < k)][7])
    full = int(inner[lens[inner] >= k][11])
    cuts = [0, 3, empty, empty + 1, short, short + 1, full + 1, lens.size - 3, lens.size]
    assert lens[empty] == 0 and 0 < lens[short] < k
    want = M.threshold(table, 2)
    _same(ctx.kmer_count(seqs, off, k, 2), want, "one piece")
    for c in cuts:
        a, b = _split(seqs, off, c)
        ctx.kmer_count_begin(k)
        ctx.kmer_count_add(*a)
        ctx.kmer_count_add(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))  # no reads: a no-op
        ctx.kmer_count_add(*b)
        _same(ctx.kmer_count_finish(2), want, "cut at read %d" % c)
    # three pieces, the middle one a single short read
    ctx.kmer_count_begin(k)
    a, b = _split(seqs, off, short)
    b1, b2 = _split(b[0], b[1], 1)
    for piece in (a, b1, b2):
        ctx.kmer_count_add(*piece)
    _same(ctx.kmer_count_finish(2), want, "a short read alone")


def test_state_errors_and_refused_k(ctx, oracle):
    k = 3
    seqs, off, reads, table = _case("strands_and_palindromes", k)
    _same(ctx.kmer_count(seqs, off, k, 1), table)
    with pytest.raises(_lib.FedrannHipError, match=STATE):
        ctx.kmer_count_finish(1)  # (no begin: the call above finished)
    with pytest.raises(_lib.FedrannHipError, match=STATE):
        ctx.kmer_count_add(seqs, off)  # (after a fetch)
    with pytest.raises(_lib.FedrannHipError, match=STATE):
        ctx.kmer_count_export_dev(0, 1)
    ctx.kmer_count_begin(k)
    ctx.kmer_count_add(seqs, off)
    _same(ctx.kmer_count_finish(1), table, "begin / add / finish after the state errors")
    with pytest.raises(_lib.FedrannHipError, match=STATE):
        ctx.kmer_count_finish(1)  # (twice)
    lib = oracle.kmer_library(b"ACG CGT TTT AAC AAA", 3)
    for bad in (0, 32, -1, 33):
        with pytest.raises(_lib.FedrannHipError, match=r"k must be in \[1, 31\]"):
            ctx.kmer_count(seqs, off, bad, 1)
        with pytest.raises(_lib.FedrannHipError, match=r"k must be in \[1, 31\]"):
            ctx.kmer_count_begin(bad)
        with pytest.raises(_lib.FedrannHipError, match=STATE):
            ctx.kmer_count_add(seqs, off)  # (the refused begin began nothing)
        with pytest.raises(_lib.FedrannHipError, match=r"k must be in \[1, 31\]"):
            ctx.kmer_search(seqs, off, lib, bad)
        _same(ctx.kmer_count(seqs, off, k, 2), M.threshold(table, 2), "after a refused k")
        ip, ix = ctx.kmer_search(seqs, off, lib, 3)
        wp, wx = oracle.kmer_search(reads, lib, 3)
        assert np.array_equal(ip, wp) and np.array_equal(ix, wx)
    # a refused begin in the middle of a count leaves the count as it was
    a, b = _split(seqs, off, 9)
    ctx.kmer_count_begin(k)
    ctx.kmer_count_add(*a)
    with pytest.raises(_lib.FedrannHipError, match=r"k must be in \[1, 31\]"):
        ctx.kmer_count_begin(32)
    ctx.kmer_count_add(*b)
    _same(ctx.kmer_count_finish(1), table, "a refused begin under way")


# ---- large counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", M.KS)
def test_homopolymers_land_on_code_zero_with_every_window(ctx, k):
    reads = list(M.HOMOPOLYMERS)
    seqs, off = M.from_reads(reads)
    n = M.homopolymer_count(k)
    want = (np.zeros(1, dtype=np.uint64), np.array([n], dtype=np.uint64))
    _same(M.string_count(reads, k, 1), want, "the model")
    _same(ctx.kmer_count(seqs, off, k, 1), want)
    _same(ctx.kmer_count(seqs, off, k, n), want, "min_count = the count")
    assert ctx.kmer_count(seqs, off, k, n + 1)[0].size == 0
    s4, o4 = M.from_reads(reads * 4)
    try:
        ctx.set_kmer_count_block(seqs.size + 1)
        _same(ctx.kmer_count(s4, o4, k, 1), (want[0], want[1] * np.uint64(4)), "four blocks")
        assert ctx.last_kmer_count_blocks() == 4
    finally:
        ctx.set_kmer_count_block(0)
