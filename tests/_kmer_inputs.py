"""Inputs for the k-mer search tests against the reference's own kmer_searcher (test_kmer_reference.py,
test_gpu_kmer_reference.py): small FASTA / FASTQ files and libraries that mix every rule of its reader, its
library loader and its scan, and helpers that turn its output into the CSR the product returns."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def random_bases(rng, n):
    return ACGT[rng.integers(0, 4, size=int(n))].tobytes()


def palindromes(rng, k, n):
    """n k-mers equal to their own reverse complement (even k only)."""
    out = []
    for _ in range(n):
        h = random_bases(rng, k // 2)
        out.append(h + revcomp(h))
    return out


def rows_to_csr(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if rows else np.zeros(0, np.int64)
    return indptr, indices


def write_fasta(path, ids, reads):
    with open(path, "wb") as f:
        f.write(b"".join(b">%s\n%s\n" % (i, r) for i, r in zip(ids, reads)))


def library_text(rng, fwd, k, junk=True):
    """`cat fwd rev` as the reference's pipeline feeds it: the forward k-mers, then their reverse complements
    (a palindrome's second copy takes no index).  junk: '>count' lines, '\\r\\n', tabs, blank lines, tokens of the
    wrong length, with N, in lower case, and repeats."""
    toks = list(fwd) + [revcomp(t) for t in fwd]
    if junk:
        extra = []
        for t in toks:
            u = rng.random()
            if u < 0.05:
                extra.append(t.lower())  # a repeat in lower case
            elif u < 0.10 and len(t) > 0:
                p = int(rng.integers(0, len(t)))
                extra.append(t[:p] + b"N" + t[p + 1:])
            elif u < 0.15:
                extra.append(t + b"A")
            elif u < 0.20 and len(t) > 1:
                extra.append(t[1:])
            elif u < 0.25:
                extra.append(b">%d" % int(rng.integers(1, 10 ** min(k, 9))))
        for t in extra:
            toks.insert(int(rng.integers(0, len(toks) + 1)), t)
    seps = [b"\n", b"\r\n", b" ", b"\t", b"\n\n", b" \r\n"]
    out = []
    for t in toks:
        out.append(t)
        out.append(seps[int(rng.integers(0, len(seps)))] if junk else b"\n")
    return b"".join(out)


def _mutate(rng, s, k):
    s = bytearray(s)
    for p in range(len(s)):
        u = rng.random()
        if u < 0.03:
            s[p] = ord("N")
        elif u < 0.08:
            s[p] |= 0x20
    return bytes(s)


def random_case(rng, k, fastq):
    """One small reads file (FASTA or FASTQ) and one library text at k.  Library: windows of a random genome,
    T^(k-j) + X k-mers (what a window reads just after an invalid character), A-padded short reads (what a read
    shorter than k looks up), palindromes at even k; reads: pieces of the genome and of the library k-mers behind
    N, lengths 0, 1, k - 1, k, k + 1 and longer, N and lower case, '\\r' line ends."""
    genome = random_bases(rng, 3000)
    fwd = [genome[p:p + k] for p in rng.integers(0, len(genome) - k, size=40)]
    reads = []
    for _ in range(int(rng.integers(15, 40))):
        u = rng.random()
        if u < 0.35:
            n = int(rng.choice([0, 1, max(k - 1, 0), k, k + 1]))
        else:
            n = int(rng.integers(0, 3 * k + 20))
        a = int(rng.integers(0, len(genome) - n))
        r = genome[a:a + n]
        if n and rng.random() < 0.4:  # N followed by the tail of a T-prefixed library k-mer
            j = int(rng.integers(1, k)) if k > 1 else 1
            x = random_bases(rng, j)
            fwd.append((b"T" * (k - j) + x)[-k:])
            p = int(rng.integers(0, n + 1))
            r = r[:p] + b"N" + x + r[p:]
        if 0 < len(r) < k and rng.random() < 0.5:
            fwd.append(b"A" * (k - len(r)) + r.upper().replace(b"N", b"A"))
        reads.append(_mutate(rng, r, k))
    if k % 2 == 0:
        pal = palindromes(rng, k, 6)
        fwd += pal
        for p in pal:
            reads.append(random_bases(rng, int(rng.integers(0, 5))) + p + random_bases(rng, int(rng.integers(0, 5))))
    if rng.random() < 0.3:
        fwd.append(b"A" * k)  # the code an empty read looks up
    rng.shuffle(fwd)
    lib = library_text(rng, fwd, k)
    ids = [b"r%d" % i for i in range(len(reads))]
    return (fastq_text(rng, ids, reads) if fastq else fasta_text(rng, ids, reads)), lib


def fasta_text(rng, ids, reads):
    out = []
    if rng.random() < 0.3:
        out.append(b"\n")  # a blank first line: still FASTA
    if rng.random() < 0.3:
        out.append(random_bases(rng, 20) + b"\n")  # sequence before the first header: dropped
    for name, r in zip(ids, reads):
        u = rng.random()
        if u < 0.05:
            out.append(b">\n" + random_bases(rng, 10) + b"\n")  # an empty id: the record is dropped
        elif u < 0.1:
            out.append(b"> desc only\n" + random_bases(rng, 10) + b"\n")
        v = rng.random()
        head = b">" + name + (b"" if v < 0.4 else b" some desc" if v < 0.6 else b"\tx y" if v < 0.8 else b" d\r")
        out.append(head + b"\n")
        p = 0
        while p < len(r):
            w = int(rng.integers(1, 40))
            line = r[p:p + w]
            p += w
            if rng.random() < 0.15:
                line += b"\r"  # stays in the sequence: an invalid character
            out.append(line + b"\n")
            if rng.random() < 0.1:
                out.append(b"\n")
    text = b"".join(out)
    return text[:-1] if rng.random() < 0.3 else text  # with or without a final '\n'


def fastq_text(rng, ids, reads):
    out = []
    for name, r in zip(ids, reads):
        v = rng.random()
        head = b"@" + name + (b"" if v < 0.5 else b" with spaces" if v < 0.8 else b"  two  spaces")
        if rng.random() < 0.1:
            r = r + b"\r"
        qual = bytes(rng.choice(list(b"!@I#"), size=len(r)).astype(np.uint8))  # may start with '@'
        out.append(head + b"\n" + r + b"\n+\n" + qual + b"\n")
        if rng.random() < 0.1:
            out.append(b"\n")
    return b"".join(out)
