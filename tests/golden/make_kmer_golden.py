"""Generate the k-mer search fixtures tests/golden/kmer_* by RUNNING the reference's kmer_searcher.

Run in the build container after build() (which compiles kmer_searcher.cpp from the reference checkout into
oracle/_ref/kmer_searcher against oracle/ref_shim/robin_hood.h; see oracle/Makefile):

    python -B tests/golden/make_kmer_golden.py [REFERENCE_CHECKOUT]

What is produced (data only: inputs + the program's outputs, no reference source):

  kmer_test1.{fastq,kmers.txt}   the reference's own test data (kmer_searcher/test/data/), copied
  kmer_test2.{fasta,kmers.txt}
  kmer_quirks_fa.{fasta,kmers.txt}   hand-made: every rule of the FASTA reader, the library loader and the scan
  kmer_quirks_fq.{fastq,kmers.txt}   hand-made: the FASTQ reader (see the comments at QUIRK_CASES)
  kmer_<case>.output.bin         output.bin of `kmer_searcher <kmers> <reads> OUT <k> 1`, each record's indices
                                 sorted ascending (the program writes them in its hash set's order, which the
                                 stand-in header changes and the reference leaves unspecified)
  kmer_<case>.kmer_frequency.bin kmer_frequency.bin of the same run, as written
  kmer_cases.json                case -> reads file, library file, k

tests/test_kmer_reference.py checks that the live binary still writes these bytes and that the oracle and the
product's host code agree with them.
"""
import json
import os
import shutil
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

# FASTA, k = 4: a blank first line (still FASTA), sequence before the first header, empty ids ('>' and '> desc':
# the record is dropped with its sequence), ids cut at a space or a tab, '\r\n' line ends ('\r' stays in the
# sequence as an invalid character; a header's '\r' must follow a space, or the program refuses the id), blank
# lines inside a record, lower case, reads of length 0, 1, k - 1, k, k + 1, windows after an N that hit the
# T-prefixed library k-mers TTTA / TTAC / TACG, the palindrome ACGT.  Library: '>count' lines left in, '\r\n',
# tokens of the wrong length, with N, in lower case, duplicated (the duplicate takes no index), AAAA (the code an
# empty read looks up) and AACG (a read of length 2 'CG' looks up A-padded AACG).
QUIRKS_FA = (b"\n"
             b"ACGTACGT\n"
             b">empty0\n"
             b">r1 some description\r\n"
             b"ACGTNACGT\r\n"
             b"\n"
             b"TTACGtacg\n"
             b">\n"
             b"ACGTACGT\n"
             b"> only a description\n"
             b"TTTT\n"
             b">r2\tx\n"
             b"NACG\n"
             b">r3\n"
             b"C\n"
             b">r4\n"
             b"CG\n"
             b">r5 d\r\n"
             b"ACG\r\n"
             b">r6\n"
             b"acgta\n"
             b">r7\n"
             b">r8\n"
             b"GGNNTACGTTAC\n"
             b"TTTANCGC\n"
             b">r9\n"
             b"ACGT")
QUIRKS_FA_LIB = (b">12\r\nACGT\r\n>3\r\nTTTA\r\nttac\n\n  TACG\tACG ACGTA acNt\n>4\nACGT\nCGCA\nAAAA\nAACG\nTACG\n"
                 b"GTAC\nCCCC\n")

# FASTQ, k = 3: headers with spaces (the stand-alone program keeps the whole line as the id), quality
# lines that start with '@' (skipped with the '+' line), blank lines between records, a '\r' at the end of a
# sequence line, reads of length 0, 1, 2, 3, 4, N runs, lower case.
QUIRKS_FQ = (b"@q1 first read\n"
             b"ACGTT\n+\n@@@@@\n"
             b"\n"
             b"@q2  two  spaces\n"
             b"\n+\n\n"
             b"@q3\n"
             b"A\n+\n@\n"
             b"@q4 two\n"
             b"NT\n+q4\n!!\n"
             b"\n\n"
             b"@q5\n"
             b"TTA\r\n+\n!!!!\n"
             b"@q6 x y z\n"
             b"acgNNNTAC\n+\n@@@@@@@@@\n"
             b"@q7\n"
             b"GGGTTTTG\n+\n!!!!!!!!\n")
QUIRKS_FQ_LIB = b">1\nAAA\nTTA\nTAC\nACG\nacg\nCGT\nGTT\nAAT\nTTT\nTTG\nGGT\nAN\nACGT\n>2\nTTC\n"

REF_CASES = {  # case -> (reads file, library file, k) in kmer_searcher/test/data/, as test/test.sh runs them
    "test1": ("test1.fastq", "test1.kmers.txt", 15),
    "test2": ("test2.fasta", "test2.kmers.txt", 13),
}
QUIRK_CASES = {
    "quirks_fa": (QUIRKS_FA, "fasta", QUIRKS_FA_LIB, 4),
    "quirks_fq": (QUIRKS_FQ, "fastq", QUIRKS_FQ_LIB, 3),
}


def sorted_output_bin(ids, rows):
    out = [struct.pack("<4sB3sQ", b"KMER", 1, b"\0\0\0", len(ids))]
    for name, r in zip(ids, rows):
        out.append(struct.pack("<H", len(name)) + name + struct.pack("<I", len(r)) + r.astype("<u8").tobytes())
    return b"".join(out)


def main(ref):
    from oracle import oracle
    data = os.path.join(ref, "kmer_searcher", "test", "data")
    cases = {}
    for case, (reads, lib, k) in REF_CASES.items():
        ext = reads.rsplit(".", 1)[1]
        shutil.copyfile(os.path.join(data, reads), os.path.join(HERE, "kmer_%s.%s" % (case, ext)))
        shutil.copyfile(os.path.join(data, lib), os.path.join(HERE, "kmer_%s.kmers.txt" % case))
        cases[case] = {"reads": "kmer_%s.%s" % (case, ext), "kmers": "kmer_%s.kmers.txt" % case, "k": k}
    for case, (reads, ext, lib, k) in QUIRK_CASES.items():
        with open(os.path.join(HERE, "kmer_%s.%s" % (case, ext)), "wb") as f:
            f.write(reads)
        with open(os.path.join(HERE, "kmer_%s.kmers.txt" % case), "wb") as f:
            f.write(lib)
        cases[case] = {"reads": "kmer_%s.%s" % (case, ext), "kmers": "kmer_%s.kmers.txt" % case, "k": k}
    for case, c in cases.items():
        with tempfile.TemporaryDirectory() as tmp:
            ids, rows, freq = oracle.run_kmer_searcher(os.path.join(HERE, c["kmers"]), os.path.join(HERE, c["reads"]),
                                                       tmp, c["k"])
        with open(os.path.join(HERE, "kmer_%s.output.bin" % case), "wb") as f:
            f.write(sorted_output_bin(ids, rows))
        with open(os.path.join(HERE, "kmer_%s.kmer_frequency.bin" % case), "wb") as f:
            f.write(freq)
        print(case, "k=%d" % c["k"], [(i.decode(), r.tolist()) for i, r in zip(ids, rows)])
    with open(os.path.join(HERE, "kmer_cases.json"), "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
