"""The k-mer counting tests' own ground, checked without the product: oracle.kmer_count (a numpy restatement with
shifts and masks) against _kmer_count_model.string_count (byte strings, no shifts) on every input builder, and the
builders' claims about the edges they hold."""
import numpy as np
import pytest

import _kmer_count_model as M
from _kmer_inputs import revcomp

MIN_COUNTS = (0, 1, 2, 5)


def _builders(k):
    return {
        "boundary_reads": M.boundary_reads(np.random.default_rng(40 + k), k),
        "placed_invalids": M.placed_invalids(k),
        "byte_values": M.byte_values(),
        "strands_and_palindromes": M.strands_and_palindromes(np.random.default_rng(60 + k), k),
    }


@pytest.mark.parametrize("k", M.KS)
def test_oracle_count_equals_the_string_model_on_every_builder(oracle, k):
    for name, (seqs, off, _) in _builders(k).items():
        reads = M.to_reads(seqs, off)
        for min_count in MIN_COUNTS:
            wc, wn = M.string_count(reads, k, min_count)
            oc, on = oracle.kmer_count(reads, k, min_count)
            assert np.array_equal(oc, wc) and np.array_equal(on, wn), (name, min_count)
            assert wc.dtype == np.uint64 and wn.dtype == np.uint64
        assert M.string_count(reads, k, 1)[0].size > 0, name


def test_the_string_model_on_reads_counted_by_hand():
    c, n = M.string_count([b"ACGT", b"", b"AC", b"ANTTTA", b"acgt", b"NA"], 2, 1)
    # AC CG GT | AC | TT TT TA | ac cg gt: AC = GT -> 0b0001 x 5, CG x 2, AA = TT -> 0 x 2, TA -> 0b1100 x 1
    assert c.tolist() == [0, 1, 6, 12] and n.tolist() == [2, 5, 2, 1]
    assert M.string_count([b"ACGT"], 2, 3)[0].tolist() == []
    assert M.string_count([b"ACGT"], 2, 0)[1].tolist() == M.string_count([b"ACGT"], 2, -4)[1].tolist() == [2, 1]
    c, n = M.string_count([b"G" * 31], 31, 1)  # CCC...C is the smaller: code 0b0101...01
    assert c.tolist() == [(4 ** 31 - 1) // 3] and n.tolist() == [1]
    assert M.string_count([b"ACG"], 4, 1)[0].size == 0 and M.string_count([], 1, 1)[0].size == 0


@pytest.mark.parametrize("k", M.KS)
def test_boundary_reads_hold_the_edges(k):
    seqs, off, e = M.boundary_reads(np.random.default_rng(40 + k), k)
    assert e == M.boundary_edges(off, k) and e["total"] == seqs.size
    assert 36_864 < e["total"] < 45_000 and e["chunks"] >= 9
    assert {0, 1, k - 1, k, k + 1, 2 * k} <= e["lengths"] and max(e["lengths"]) <= 2 * k + 5
    assert e["start_mod_stretch"] == set(range(16))
    assert e["chunk_start_d"] == {0, 1, k - 2, k - 1, k}
    assert e["most_starts_in_a_stretch"] >= 3
    assert e["empty_run_at_start"] >= 3 and e["empty_run_at_chunk"] >= 3 and e["empty_run_at_end"] >= 3
    assert set(np.unique(seqs).tolist()) == set(b"ACGT")
    if k >= 15:  # both strands of the genome: some k-mer of one read occurs reverse-complemented in another
        reads = [r for r in M.to_reads(seqs, off) if len(r) >= k]
        fw = {r[i:i + k] for r in reads for i in range(len(r) - k + 1)}
        assert any(revcomp(w) in fw for w in fw)


@pytest.mark.parametrize("k", M.KS)
def test_placed_invalids_sit_where_they_are_named(k):
    seqs, off, e = M.placed_invalids(k)
    want = {"c0-1": (-1,), "c0": (0,), "c0+1": (1,), "c0-k,c0": (-k, 0), "c0-(k-1),c0": (1 - k, 0),
            "c0-1,c0-1+(k-1)": (-1, k - 2), "c0-1,c0-1+k": (-1, k - 1),
            "p0-(k-1)": (1 - k,), "p0-k": (-k,), "p0-1": (-1,), "p0": (0,), "p0-k,p0": (-k, 0),
            "p0-(k-1),p0": (1 - k, 0), "p0,p0+(k-1)": (0, k - 1), "p0,p0+k": (0, k)}
    assert [p[0] for p in e["places"]] == [n for n in want if n[0] == "p"] + ["first byte", "last byte"] + \
        [n for n in want if n[0] == "c"]
    assert len(e["places"]) == off.size - 1 and seqs.size < 100_000
    valid = np.isin(seqs, np.frombuffer(b"ACGT", dtype=np.uint8))
    for name, r, anchor, at in e["places"]:
        lo, hi = int(off[r]), int(off[r + 1])
        assert np.flatnonzero(~valid[lo:hi]).tolist() == [a - lo for a in at], name  # these and no other
        if name == "first byte":
            assert at == (lo,)
        elif name == "last byte":
            assert at == (hi - 1,)
        else:
            assert at == tuple(sorted({anchor + d for d in want[name]})), name
            assert anchor % M.STRETCH == 0 and (anchor % M.CHUNK == 0) == (name[0] == "c"), name
            # whole valid windows on both sides, and the chunk's 32 bytes of history inside the read
            assert at[0] - lo >= max(k, 32) and hi - 1 - at[-1] >= k, name


def test_byte_values_hold_every_byte_once_between_valid_flanks():
    seqs, off, e = M.byte_values()
    reads = M.to_reads(seqs, off)
    assert len(reads) == 256 and seqs.size < 100_000
    for v, (r, (a, b)) in enumerate(zip(reads, e["flanks"].tolist())):
        assert r[a] == v and len(r) == a + 1 + b and min(a, b) >= 32
        assert not (r[:a] + r[a + 1:]).translate(None, b"ACGT")
    assert M.BASES == set(b"ACGTacgt")
    for k in M.KS:  # only ACGTacgt join their flanks: the number of windows says which bytes were taken as bases
        for v, (r, (a, b)) in enumerate(zip(reads, e["flanks"].tolist())):
            n = int(M.string_count([r], k, 1)[1].sum())
            assert n == (a + 1 + b - k + 1 if v in M.BASES else (a - k + 1) + (b - k + 1)), (k, v)


@pytest.mark.parametrize("k", M.KS)
def test_strand_reads_hold_what_they_are_about(k):
    seqs, off, kinds = M.strands_and_palindromes(np.random.default_rng(60 + k), k)
    reads = M.to_reads(seqs, off)
    assert seqs.size < 100_000
    assert len(kinds["forward"]) == len(kinds["reverse"]) == 12
    for f, r in zip(kinds["forward"], kinds["reverse"]):
        assert reads[r] == revcomp(reads[f]) and len(reads[f]) >= 3 * k
        if k >= 15:  # a k-mer of the one read is in the other only reverse-complemented
            w = reads[f][3:3 + k]
            assert w != revcomp(w) and w not in reads[r] and revcomp(w) in reads[r]
    assert (len(kinds["palindrome"]) == 8) == (k % 2 == 0) and (len(kinds["palindrome"]) == 0) == (k % 2 == 1)
    for p in kinds["palindrome"]:
        assert any(reads[p][i:i + k] == revcomp(reads[p][i:i + k]) for i in range(len(reads[p]) - k + 1))
    assert [reads[h] for h in kinds["homopolymer"]] == [b"A" * 20000, b"T" * 15000, b"a" * 7]
    assert sorted(reads[p] for p in kinds["pair"]) == sorted(bytes([a, b]) for a in b"ACGT" for b in b"ACGT")
    # the homopolymers alone: one code, 0, with every window of the three reads
    c, n = M.string_count([reads[h] for h in kinds["homopolymer"]], k, 1)
    assert c.tolist() == [0] and n.tolist() == [M.homopolymer_count(k)]
    assert M.homopolymer_count(k) == (20001 - k) + (15001 - k) + max(0, 8 - k)
    if k % 2 == 0:  # a palindrome counts once per window, not once per strand
        p = reads[kinds["palindrome"][0]]
        assert int(M.string_count([p], k, 1)[1].sum()) == len(p) - k + 1


@pytest.mark.parametrize("k", [1, 3, 16, 31])
def test_tiling_multiplies_the_oracles_counts(oracle, k):
    base_seqs, base_off = M.grid_stride_base(k)
    assert int(base_off[-1]) % 16 != 0 and base_seqs.size < 100_000
    base = oracle.kmer_count(M.to_reads(base_seqs, base_off), k, 1)
    seqs, off, e = M.tiled(base_seqs, base_off, 3)
    assert e == {"times": 3, "base_total": int(base_off[-1]), "total": seqs.size, "copy_shifts": 3}
    assert off.size == 3 * (base_off.size - 1) + 1 and int(off[-1]) == seqs.size
    assert M.to_reads(seqs, off) == 3 * M.to_reads(base_seqs, base_off)
    tail = [b"ACGTTGCATTAGGACCAGTACCGATTAGACCATTTGACA"]
    for min_count in (1, 2, 5):
        got = oracle.kmer_count(M.to_reads(seqs, off) + tail, k, min_count)
        want = M.threshold(M.merge_tables(M.scale_table(base, 3), oracle.kmer_count(tail, k, 1)), min_count)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(AssertionError, match="whole stretches"):
        M.tiled(np.zeros(32, np.uint8), np.array([0, 32], dtype=np.int64), 2)


def test_times_to_exceed():
    assert M.times_to_exceed(10, 99) == 10 and M.times_to_exceed(10, 100) == 11 and M.times_to_exceed(10, 101) == 11
