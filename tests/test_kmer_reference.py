"""The k-mer search's host side against the reference program itself (no GPU): oracle/_ref/kmer_searcher is
kmer_searcher/kmer_searcher.cpp compiled unchanged by build() (oracle/Makefile, with oracle/ref_shim/robin_hood.h
for the un-vendored hash map).  It runs with 1 thread, so its records come in file order; a record's indices are
in hash-set order, which the reference leaves unspecified, so they are sorted before comparing.

The oracle's restatement (read_sequences + kmer_library + kmer_search) and the product's native reader and
library loader (kmer_search.read_sequences, load_kmer_library) must give the program's ids, record count, index
sets and kmer_frequency.bin bytes.  The stand-alone program keeps a FASTQ header's whole line as the id
(fastq_ids_as_fasta=False); the pipeline's `seqkit fq2fa` rule is covered in test_kmer_host.py."""
import json

import numpy as np
import pytest

from fedrann_amd import kmer_search as ks

from _kmer_inputs import random_case
from conftest import golden

CASES = json.load(open(golden("kmer_cases.json")))


def _host(oracle, reads_path, lib_path, k, tmp_path):
    """(ids, sorted index rows, output.bin bytes, kmer_frequency.bin bytes) from the oracle and from the product's
    host code (its reader and loader; the CPU search is the oracle's); the two must agree."""
    with open(lib_path, "rb") as f:
        text = f.read()
    o_ids, o_seqs = oracle.read_sequences(str(reads_path))
    o_codes = oracle.kmer_library(text, k)
    ids, seqs, off = ks.read_sequences(str(reads_path), fastq_ids_as_fasta=False)
    codes = ks.load_kmer_library(text, k)
    assert ids == o_ids, "native reader and oracle disagree on the ids"
    assert [bytes(seqs[off[i]:off[i + 1]]) for i in range(len(ids))] == o_seqs
    assert np.array_equal(codes, o_codes), "native library loader and oracle disagree"
    indptr, indices = oracle.kmer_search(o_seqs, o_codes, k)
    rows = [indices[indptr[i]:indptr[i + 1]].astype(np.uint64) for i in range(len(ids))]
    ks.write_output_bin(str(tmp_path / "host.bin"), ids, indptr, indices)
    ks.write_kmer_frequency_bin(str(tmp_path / "host_freq.bin"), indices, codes.size)
    return ids, rows, (tmp_path / "host.bin").read_bytes(), (tmp_path / "host_freq.bin").read_bytes()


def _assert_same(got, want_ids, want_rows, want_freq, what):
    ids, rows, _, freq = got
    assert len(ids) == len(want_ids), "%s: %d records, the reference wrote %d" % (what, len(ids), len(want_ids))
    assert ids == want_ids, "%s: ids differ" % what
    for r, (a, b) in enumerate(zip(rows, want_rows)):
        assert np.array_equal(a, b), "%s: record %d (%r): %s, reference %s" % (what, r, ids[r], a, b)
    assert freq == want_freq, "%s: kmer_frequency.bin differs" % what


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_matches_recorded_reference_output(oracle, tmp_path, case):
    """The fixtures made by the reference program (tests/golden/make_kmer_golden.py): output.bin with each record
    sorted equals, byte for byte, what the product's writer makes from the oracle's search."""
    c = CASES[case]
    got = _host(oracle, golden(c["reads"]), golden(c["kmers"]), c["k"], tmp_path)
    with open(golden("kmer_%s.output.bin" % case), "rb") as f:
        assert got[2] == f.read(), "output.bin differs from the reference's (indices sorted per record)"
    want_ids, want_rows = oracle.read_kmer_output(golden("kmer_%s.output.bin" % case))
    with open(golden("kmer_%s.kmer_frequency.bin" % case), "rb") as f:
        _assert_same(got, want_ids, want_rows, f.read(), case)


@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_binary_reproduces_fixtures(oracle, tmp_path, case):
    """The program build() compiled is the one that recorded tests/golden/kmer_*."""
    c = CASES[case]
    ids, rows, freq = oracle.run_kmer_searcher(golden(c["kmers"]), golden(c["reads"]), tmp_path, c["k"])
    want_ids, want_rows = oracle.read_kmer_output(golden("kmer_%s.output.bin" % case))
    assert ids == want_ids
    assert all(np.array_equal(a, b) for a, b in zip(rows, want_rows))
    with open(golden("kmer_%s.kmer_frequency.bin" % case), "rb") as f:
        assert freq == f.read()


def test_reference_test_data_by_hand():
    """The reference's own test1 (k = 15), worked by hand: r1 holds library k-mers 2 and 4, r2 holds 4."""
    from oracle import oracle
    ids, rows = oracle.read_kmer_output(golden("kmer_test1.output.bin"))
    assert ids == [b"r1", b"r2"] and [r.tolist() for r in rows] == [[2, 4], [4]]
    freq = np.fromfile(golden("kmer_test1.kmer_frequency.bin"), dtype="<u8").reshape(-1, 2)
    assert freq.tolist() == [[2, 1], [4, 2]]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 15, 16, 31])
def test_random_small_files_against_reference_binary(oracle, tmp_path, k):
    """Seeded random FASTA and FASTQ files and libraries that mix every rule (see _kmer_inputs.random_case),
    run through the live reference program with 1 thread."""
    for seed in range(12):
        rng = np.random.default_rng(1000 * k + seed)
        fastq = seed % 2 == 1
        reads, lib = random_case(rng, k, fastq)
        rp, lp = tmp_path / ("r%d.%s" % (seed, "fq" if fastq else "fa")), tmp_path / ("l%d.txt" % seed)
        rp.write_bytes(reads)
        lp.write_bytes(lib)
        want_ids, want_rows, want_freq = oracle.run_kmer_searcher(lp, rp, tmp_path / ("o%d" % seed), k)
        got = _host(oracle, rp, lp, k, tmp_path)
        _assert_same(got, want_ids, want_rows, want_freq, "k=%d seed=%d %s" % (k, seed, "FASTQ" if fastq else "FASTA"))
        assert sum(len(r) for r in want_rows) > 0, "k=%d seed=%d: the library is never hit" % (k, seed)
