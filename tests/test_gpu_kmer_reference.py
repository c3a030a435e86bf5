"""fdr_kmer_search (GPU) and the drop-in kmer_search.kmer_searcher() against the reference program itself:
oracle/_ref/kmer_searcher, kmer_searcher/kmer_searcher.cpp compiled unchanged by build() (see
test_kmer_reference.py), run with 1 thread.  Each record's indices are sorted before comparing (the program
writes them in hash-set order, which the reference leaves unspecified).

The inputs aim at the kernel's edges: ks_search_kernel stages 4 KiB chunks with 32 bytes of history and gives
each thread 16 window ends; reads shorter than k go to ks_short_reads_kernel; the hit buffer is sized by a guess
(max(2^20, positions / 4 + reads)) and the pass rerun when it was too small."""
import numpy as np
import pytest

from fedrann_amd import feature_extraction as fx
from fedrann_amd import kmer_search as ks

from _kmer_inputs import ACGT, palindromes, revcomp, rows_to_csr, write_fasta

pytestmark = pytest.mark.gpu


def _reads(seqs, off):
    return [bytes(seqs[off[i]:off[i + 1]]) for i in range(off.size - 1)]


def _reference(oracle, tmp_path, lib_text, reads, k, ids=None):
    """The program's (ids, CSR) for these reads (written as FASTA, one line per read) and library text."""
    ids = ids or [b"r%d" % i for i in range(len(reads))]
    (tmp_path / "lib.txt").write_bytes(lib_text)
    write_fasta(str(tmp_path / "reads.fa"), ids, reads)
    got_ids, rows, _ = oracle.run_kmer_searcher(tmp_path / "lib.txt", tmp_path / "reads.fa", tmp_path / "ref", k,
                                                expect_records=len(ids))
    assert got_ids == ids
    return rows_to_csr(rows)


def _assert_gpu_equals_reference(ctx, oracle, tmp_path, seqs, off, lib_text, k, min_hits):
    codes = ks.load_kmer_library(lib_text, k)
    wp, wx = _reference(oracle, tmp_path, lib_text, _reads(seqs, off), k)
    ip, ix = ctx.kmer_search(seqs, off, codes, k)
    assert np.array_equal(ip, wp), "row pointers differ from the reference program's"
    assert np.array_equal(ix.astype(np.int64), wx), "library indices differ from the reference program's"
    assert wx.size >= min_hits, "the reference finds only %d hits" % wx.size


def _t_prefixed(seqs, q, k, rng):
    """Library k-mers T^(k-j) + the j characters after an invalid character at q: what the window ending j
    characters later reads."""
    out = []
    for j in rng.integers(1, k, size=2) if k > 1 else [1]:
        x = bytes(seqs[q + 1:q + 1 + int(j)]).upper()
        out.append(b"T" * (k - len(x)) + x)
    return out


@pytest.mark.parametrize("k", [31, 16, 5])
def test_n_at_every_chunk_offset_with_t_prefixed_library(ctx, oracle, tmp_path, k):
    """An N every 65 characters (gcd(65, 4096) = 1: over 4096 of them it falls on every offset of a 4 KiB chunk and
    so of every 16-position thread stretch), a library dense in the T^(k-j) + X k-mers the windows after it read,
    plus windows of the reads, in reads of 1.5 - 12 kbases that cross chunk boundaries; some lower case."""
    rng = np.random.default_rng(70 + k)
    total = 65 * 4200
    seqs = ACGT[rng.integers(0, 4, size=total)].copy()
    n_pos = np.arange(11, total - k - 1, 65)
    seqs[n_pos] = ord("N")
    lens = []
    while sum(lens) < total:
        lens.append(int(rng.integers(1500, 12000)))
    lens[-1] -= sum(lens) - total
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    lib = []
    for q in n_pos.tolist():
        lib += _t_prefixed(seqs, q, k, rng)
    for p in rng.integers(0, total - k, size=total // 40).tolist():
        w = bytes(seqs[p:p + k])
        if b"N" not in w:
            lib.append(w)
    seqs[rng.random(total) < 0.01] |= 0x20
    _assert_gpu_equals_reference(ctx, oracle, tmp_path, seqs, off, b"\n".join(lib) + b"\n", k, min_hits=4000)


@pytest.mark.parametrize("k", [31, 16, 5])
def test_thousands_of_short_reads(ctx, oracle, tmp_path, k):
    """20 000 reads of length 0 ... k + 1 side by side (ks_short_reads_kernel for those below k, read boundaries
    everywhere in the chunks and stretches of ks_search_kernel for the others); the library holds the A-padded codes
    of half the short reads, the T-prefixed k-mers after their N, and code 0 (what an empty read looks up)."""
    rng = np.random.default_rng(80 + k)
    lens = rng.integers(0, k + 2, size=20_000)
    reads, lib = [], [b"A" * k]
    for n in lens.tolist():
        r = bytearray(ACGT[rng.integers(0, 4, size=n)].tobytes())
        if n and rng.random() < 0.1:
            r[int(rng.integers(0, n))] = ord("N")
        r = bytes(r)
        if rng.random() < 0.5:
            p = r.rfind(b"N")
            if p < 0:
                lib.append(b"A" * (k - n) + r if n < k else r[n - k:])
            else:
                lib.append((b"T" * k + r[p + 1:])[-k:])
        if rng.random() < 0.05:
            r = r.lower()
        reads.append(r)
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    seqs = np.frombuffer(b"".join(reads), dtype=np.uint8)
    _assert_gpu_equals_reference(ctx, oracle, tmp_path, seqs, off, b"\n".join(lib) + b"\n", k, min_hits=5000)


@pytest.mark.parametrize("k", [1, 2])
def test_k1_k2_nearly_every_kmer_and_hit_buffer_rerun(ctx, oracle, tmp_path, k):
    """k = 1 and 2 with a library of nearly every k-mer (forward, then reverse: the palindromes' second copies take
    no index), over 4.5 M window positions: the hits exceed the hit buffer's first guess and the pass is rerun."""
    rng = np.random.default_rng(90 + k)
    every = [ACGT[[(c >> (2 * (k - 1 - j))) & 3 for j in range(k)]].tobytes() for c in range(4 ** k)]
    fwd = [every[i] for i in rng.permutation(len(every))[:len(every) - 1]]  # all but one
    lib = b"\n".join(fwd + [revcomp(t) for t in fwd]) + b"\n"
    lens = rng.integers(0, 900, size=10_000)
    seqs = ACGT[rng.integers(0, 4, size=int(lens.sum()))].copy()
    seqs[rng.random(seqs.size) < 0.002] = ord("N")
    seqs[rng.random(seqs.size) < 0.01] |= 0x20
    off = np.zeros(lens.size + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    assert off[-1] > 4_000_000
    _assert_gpu_equals_reference(ctx, oracle, tmp_path, seqs, off, lib, k, min_hits=20_000)


def test_drop_in_even_k_palindromes_blocks_and_streaming(ctx, oracle, tmp_path):
    """k = 16 with palindromic library k-mers (in the forward and so in the reverse library): the drop-in
    kmer_searcher() on FASTQ reads with spaces in their headers and on '>count' library files, the same reads
    through ctx.kmer_search, through kmer_search.search in small blocks and through the streamed drop-in in small
    pieces -- all against one run of the reference program: output.bin (indices sorted per record),
    kmer_frequency.bin byte for byte, and the CSR build_feature_csr reads back."""
    k = 16
    rng = np.random.default_rng(95)
    genome = ACGT[rng.integers(0, 4, size=400_000)].tobytes()
    pal = palindromes(rng, k, 300)
    fwd = [genome[p:p + k] for p in rng.integers(0, len(genome) - k, size=20_000).tolist()] + pal
    fwd = [fwd[i] for i in rng.permutation(len(fwd))]
    lens = rng.integers(0, 2500, size=2500)
    reads = []
    for n in lens.tolist():
        a = int(rng.integers(0, len(genome) - n))
        r = bytearray(genome[a:a + n])
        for _ in range(int(rng.integers(0, 3))):  # palindromes dropped in
            p = pal[int(rng.integers(0, len(pal)))]
            q = int(rng.integers(0, n + 1))
            r[q:q] = p
        for q in rng.integers(0, len(r) + 1, size=int(rng.integers(0, 3))).tolist():
            r[q:q + 1] = b"N"
        reads.append(bytes(r).lower() if rng.random() < 0.05 else bytes(r))
    ids = [b"q%d sample %d" % (i, i % 7) for i in range(len(reads))]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in zip(ids, reads)))
    fwd_p, rev_p, cat_p = tmp_path / "fwd.fasta", tmp_path / "rev.fasta", tmp_path / "cat.txt"
    fwd_p.write_bytes(b"".join(b">%d\n%s\n" % (3 + i % 5, t) for i, t in enumerate(fwd)))
    rev_p.write_bytes(b"".join(b">%d\n%s\n" % (3 + i % 5, revcomp(t)) for i, t in enumerate(fwd)))
    cat_p.write_bytes(fwd_p.read_bytes() + rev_p.read_bytes())
    w_ids, rows, w_freq = oracle.run_kmer_searcher(cat_p, fq, tmp_path / "ref", k, expect_records=len(ids))
    assert w_ids == ids
    wp, wx = rows_to_csr(rows)
    assert wx.size > 20_000
    n_fwd = ks.load_kmer_library(fwd_p.read_bytes(), k).size
    F = 2 * n_fwd

    def check(ip, ix, what):
        assert np.array_equal(ip, wp), "%s: row pointers differ from the reference program's" % what
        assert np.array_equal(np.asarray(ix, dtype=np.int64), wx), "%s: indices differ" % what

    seqs = np.frombuffer(b"".join(reads), dtype=np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    codes = ks.read_library_files([str(fwd_p), str(rev_p)], k)
    n_lib = codes.size
    assert n_lib <= F - len(set(pal))  # each palindrome's reverse copy is the same code: it takes no index
    check(*ctx.kmer_search(seqs, off, codes, k), "ctx.kmer_search")
    check(*ks.search(seqs, off, codes, k, context=ctx, block_chars=50_000), "kmer_search.search in blocks")
    ref_csr = fx.build_feature_csr(str(tmp_path / "ref" / "output.bin"), F)
    for tag, chunk in (("whole", 1 << 28), ("streamed", 30_000)):
        out = tmp_path / tag
        got_ids, ip, ix, got_n = ks.kmer_searcher([str(fwd_p), str(rev_p)], str(fq), str(out), k, context=ctx,
                                                  chunk_bytes=chunk)
        assert got_ids == ids and got_n == n_lib
        check(ip, ix, "drop-in, " + tag)
        o_ids, o_rows = oracle.read_kmer_output(str(out / "output.bin"))
        assert o_ids == ids and all(np.array_equal(a, b) for a, b in zip(o_rows, rows)), tag + ": output.bin"
        assert (out / "kmer_frequency.bin").read_bytes() == w_freq, tag + ": kmer_frequency.bin"
        got_csr = fx.build_feature_csr(str(out / "output.bin"), F)
        assert np.array_equal(got_csr[0], ref_csr[0]) and np.array_equal(got_csr[1], ref_csr[1]), tag + ": CSR"
        assert got_csr[2] == ref_csr[2] and got_csr[3] == ref_csr[3]
