"""A second witness for canonical k-mer counting, and the inputs its tests share (test_kmer_count_model.py on the
CPU, test_gpu_kmer_count.py and test_gpu_kmer.py on the GPU).

string_count states the operation on byte strings: a window counts under the lexicographically smaller of itself and
its reverse complement, which is the smaller 2-bit code because A < C < G < T.  It uses no shifts and no masks, so it
shares nothing with the kernel's registers or with oracle.kmer_count's numpy restatement.

The builders place by construction what the counting kernel's walk can get wrong: read boundaries at every offset of
the 4096-character chunks and the 16-position thread stretches, invalid bytes at the first and last byte a thread's
priming loop reads, every byte value, both strands, palindromes, homopolymers, and whole copies of a read set that
carry the same edges into the later trips of the kernel's grid-stride loop.  Each returns (seqs uint8, seq_off int64,
edges): `edges` says what the input holds, and a CPU test asserts it."""
from collections import Counter

import numpy as np

from _kmer_inputs import palindromes, random_bases, revcomp

KS = (1, 2, 3, 15, 16, 17, 30, 31)
CHUNK = 4096    # characters a workgroup stages at a time (KS_CHUNK)
STRETCH = 16    # positions one thread walks (KS_PER_THREAD)
_DIGITS = bytes.maketrans(b"ACGT", b"0123")


def string_count(reads, k, min_count=1):
    """(codes uint64 ascending, counts uint64) of the canonical k-mers of `reads` (a list of bytes) seen at least
    min_count times (min_count <= 0 acts as 1)."""
    windows = Counter()
    for r in reads:
        r = bytes(r).upper()
        windows.update(r[i:i + k] for i in range(len(r) - k + 1))
    table = Counter()
    for w, n in windows.items():
        if w.translate(None, b"ACGT"):
            continue  # a byte that is no base
        table[min(w, revcomp(w))] += n
    least = max(1, int(min_count))
    kept = sorted((int(w.translate(_DIGITS), 4), n) for w, n in table.items() if n >= least)
    return (np.array([c for c, _ in kept], dtype=np.uint64), np.array([n for _, n in kept], dtype=np.uint64))


def to_reads(seqs, seq_off):
    return [bytes(seqs[seq_off[i]:seq_off[i + 1]]) for i in range(seq_off.size - 1)]


def from_reads(reads):
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), off


def concat(*sets):
    """Several (seqs, seq_off) as one read set."""
    reads = []
    for seqs, off in sets:
        reads += to_reads(seqs, off)
    return from_reads(reads)


def scale_table(table, times):
    return table[0], table[1] * np.uint64(times)


def merge_tables(a, b):
    """The table of two read sets together, from their tables."""
    codes, inv = np.unique(np.concatenate([a[0], b[0]]), return_inverse=True)
    counts = np.zeros(codes.size, dtype=np.uint64)
    np.add.at(counts, inv, np.concatenate([a[1], b[1]]))
    return codes, counts


def threshold(table, min_count):
    keep = table[1] >= np.uint64(max(1, min_count))
    return table[0][keep], table[1][keep]


# ---- read boundaries ---------------------------------------------------------------------------------------------
def chunk_start_distances(k):
    """d for which boundary_reads starts a read at 4096 * j - d."""
    return sorted({0, 1, k - 2, k - 1, k})


def _empty_run_at(lens, off, pos):
    """Length of the longest run of empty reads that sits at character offset pos."""
    best = cur = 0
    for n, o in zip(lens.tolist(), off[:-1].tolist()):
        cur = cur + 1 if (n == 0 and o == pos) else 0
        best = max(best, cur)
    return best


def boundary_edges(seq_off, k):
    """What a read set holds of the edges boundary_reads is built for, worked out from the offsets alone.  A read
    start is the first character of a read that is not empty."""
    lens = np.diff(seq_off)
    total = int(seq_off[-1])
    starts = np.unique(seq_off[:-1][lens > 0])
    chunk_d = set()
    for d in chunk_start_distances(k):
        at = starts + d
        if np.any((at % CHUNK == 0) & (at >= CHUNK)):
            chunk_d.add(d)
    boundaries = range(CHUNK, total, CHUNK)
    return {
        "total": total,
        "chunks": (total + CHUNK - 1) // CHUNK,
        "lengths": set(lens.tolist()),
        "start_mod_stretch": set((starts % STRETCH).tolist()),
        "chunk_start_d": chunk_d,
        "most_starts_in_a_stretch": int(np.bincount(starts // STRETCH).max()),
        "empty_run_at_start": _empty_run_at(lens, seq_off, 0) if lens[0] == 0 else 0,
        "empty_run_at_chunk": max([_empty_run_at(lens, seq_off, b) for b in boundaries] or [0]),
        "empty_run_at_end": _empty_run_at(lens, seq_off, total) if lens[-1] == 0 else 0,
    }


def boundary_reads(rng, k, total=40_000):
    """About `total` characters of reads no longer than 2k + 5: pieces of a 3000-base genome, about 30 % of them
    reverse-complemented.  Lengths come from {0, 1, k-1, k, k+1, 2k} and uniform [0, 2k+6); near a chunk boundary
    4096 * j the next length is chosen so that a read starts at 4096 * j - d, d going round chunk_start_distances(k)
    with j.  Three empty reads stand at the very start, at every boundary that d = 0 hits (followed by reads of 2, 3
    and 2 characters: three starts in one stretch) and at the very end."""
    genome = random_bases(rng, 3000)
    fixed = [0, 1, max(k - 1, 0), k, k + 1, 2 * k]
    ds = chunk_start_distances(k)
    lens = [0, 0, 0]
    pos, j = 0, 1
    while pos < total:
        target = CHUNK * j - ds[(j - 1) % len(ds)]
        if pos == target:
            if ds[(j - 1) % len(ds)] == 0:
                lens += [0, 0, 0, 2, 3, 2]
                pos += 7
            else:
                n = int(rng.integers(1, 2 * k + 6))  # (not empty: the read that starts here)
                lens.append(n)
                pos += n
            j += 1
            continue
        if rng.random() < 0.4:
            n = int(fixed[int(rng.integers(0, len(fixed)))])
        else:
            n = int(rng.integers(0, 2 * k + 6))
        if 0 < target - pos < 2 * k + 6 and pos + n >= target:
            n = target - pos
        lens.append(n)
        pos += n
    lens += [0, 0, 0]
    reads = []
    for n in lens:
        a = int(rng.integers(0, len(genome) - n))
        piece = genome[a:a + n]
        reads.append(revcomp(piece) if rng.random() < 0.3 else piece)
    seqs, off = from_reads(reads)
    return seqs, off, boundary_edges(off, k)


# ---- invalid bytes at chosen places --------------------------------------------------------------------------------
def placed_invalids(k):
    """Reads of valid bases that hold one invalid byte each, or two of them k - 1 or k apart, at places named by the
    chunk start c0 (a multiple of 4096) and the stretch start p0 (a multiple of 16) they are measured from.  edges:
    "places", a list of (name, read index, c0 or p0 (for the first and last byte: the read's start), absolute positions
    of the read's invalid bytes)."""
    rng = np.random.default_rng(1000 + k)
    near_chunk = [("c0-1", (-1,)), ("c0", (0,)), ("c0+1", (1,)),
                  ("c0-k,c0", (-k, 0)), ("c0-(k-1),c0", (-(k - 1), 0)),
                  ("c0-1,c0-1+(k-1)", (-1, k - 2)), ("c0-1,c0-1+k", (-1, k - 1))]
    near_stretch = [("p0-(k-1)", (-(k - 1),)), ("p0-k", (-k,)), ("p0-1", (-1,)), ("p0", (0,)),
                    ("p0-k,p0", (-k, 0)), ("p0-(k-1),p0", (-(k - 1), 0)), ("p0,p0+(k-1)", (0, k - 1)),
                    ("p0,p0+k", (0, k))]
    reads, places = [], []
    pos = 0

    def add(name, length, anchor, rel):
        nonlocal pos
        r = bytearray(random_bases(rng, length))
        at = sorted({anchor + d for d in rel})
        for a in at:
            r[a - pos] = ord("N")
        places.append((name, len(reads), anchor, tuple(at)))
        reads.append(bytes(r))
        pos += length

    margin = 2 * k + 35  # valid bases on both sides: whole windows, and the 32 bytes of history inside the read
    for name, rel in near_stretch:
        p0 = -(-(pos + margin) // STRETCH) * STRETCH
        if p0 % CHUNK == 0:
            p0 += STRETCH  # (a stretch start that is no chunk start)
        add(name, p0 + margin + 3 - pos, p0, rel)
    add("first byte", 2 * k + 21, pos, (0,))
    add("last byte", 2 * k + 22, pos, (2 * k + 21,))
    for name, rel in near_chunk:
        c0 = -(-(pos + margin) // CHUNK) * CHUNK
        add(name, c0 + margin + 5 - pos, c0, rel)
    seqs, off = from_reads(reads)
    return seqs, off, {"places": places}


# ---- every byte value ----------------------------------------------------------------------------------------------
BASES = frozenset(b"ACGTacgt")


def byte_values():
    """256 reads: each byte value between two stretches of at least 32 valid bases (a valid k-mer on either side for
    every k up to 31).  edges: "flanks", the two lengths per read [256, 2]."""
    rng = np.random.default_rng(77)
    reads, flanks = [], []
    for v in range(256):
        a, b = 32 + v % 3, 32 + v % 5
        reads.append(random_bases(rng, a) + bytes([v]) + random_bases(rng, b))
        flanks.append((a, b))
    seqs, off = from_reads(reads)
    return seqs, off, {"flanks": np.array(flanks, dtype=np.int64)}


# ---- strands, palindromes, homopolymers ----------------------------------------------------------------------------
HOMOPOLYMERS = (b"A" * 20000, b"T" * 15000, b"a" * 7)


def strands_and_palindromes(rng, k):
    """Reads whose k-mers occur forward only next to reads that hold only their reverse complements; palindromes
    (even k); homopolymers of A, T and a; every pair of bases.  edges: the read indices of each kind."""
    reads, kinds = [], {"forward": [], "reverse": [], "palindrome": [], "homopolymer": [], "pair": []}
    for _ in range(12):
        g = random_bases(rng, 3 * k + 7)
        kinds["forward"].append(len(reads))
        reads.append(g)
        kinds["reverse"].append(len(reads))
        reads.append(revcomp(g))
    if k % 2 == 0:
        for p in palindromes(rng, k, 8):
            kinds["palindrome"].append(len(reads))
            reads.append(random_bases(rng, int(rng.integers(0, 5))) + p + random_bases(rng, int(rng.integers(0, 5))))
    for h in HOMOPOLYMERS:
        kinds["homopolymer"].append(len(reads))
        reads.append(h)
    for a in b"ACGT":
        for b in b"ACGT":
            kinds["pair"].append(len(reads))
            reads.append(bytes([a, b]))
    seqs, off = from_reads(reads)
    return seqs, off, kinds


def homopolymer_count(k):
    """Windows of the homopolymer reads: all of them count under code 0."""
    return sum(max(0, len(h) - k + 1) for h in HOMOPOLYMERS)


# ---- whole copies --------------------------------------------------------------------------------------------------
def tiled(base_seqs, base_off, times):
    """The base read set `times` times over, as whole reads.  No window crosses a read boundary, so the table of the
    tiling is the base's table with every count multiplied by `times`.  The base's total is no multiple of 16, so that
    every copy lies differently in the stretches and chunks."""
    total = int(base_off[-1])
    assert total % STRETCH != 0, "the base read set must not fill whole stretches (%d characters)" % total
    assert base_seqs.size == total
    off = np.concatenate([np.zeros(1, dtype=np.int64)] +
                         [base_off[1:] + np.int64(t) * total for t in range(times)])
    return np.tile(base_seqs, times), off, {"times": times, "base_total": total, "total": times * total,
                                            "copy_shifts": len({(t * total) % STRETCH for t in range(times)})}


def grid_stride_base(k, seed=5):
    """boundary_reads + placed_invalids as one base read set of an odd total: the copies of a tiling then lie at all
    16 offsets of a stretch in turn."""
    b = boundary_reads(np.random.default_rng(seed + k), k)
    p = placed_invalids(k)
    seqs, off = concat(b[:2], p[:2])
    if int(off[-1]) % 2 == 0:
        seqs, off = concat((seqs, off), from_reads([b"C"]))
    return seqs, off


def times_to_exceed(base_total, chars):
    """Copies of the base needed for more than `chars` characters."""
    return chars // base_total + 1
