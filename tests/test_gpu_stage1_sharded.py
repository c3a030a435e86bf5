"""The sharded stage 1 of a `--devices` run on the GPU: the W-way merge of count runs (fdr_kmer_count_merge /
_merge_dev) and the table export (fdr_kmer_count_export_dev) against numpy, and whole CLI runs whose stage-1 files and
overlaps.tsv must be the one-GPU run's byte for byte."""
import gzip
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from fedrann_amd import _lib
from fedrann_amd import __main__ as cli
from fedrann_amd.synth import synth_sequences

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def _runs(rng, W, n, lo=0, hi=1 << 40, empty=(), same=False, disjoint=False, big_counts=False):
    runs = []
    base = np.unique(rng.integers(lo, hi, size=n, dtype=np.uint64)) if same else None
    for r in range(W):
        if r in empty:
            c = np.zeros(0, dtype=np.uint64)
        elif same:
            c = base
        elif disjoint:
            w = (hi - lo) // W
            c = np.unique(rng.integers(lo + r * w, lo + (r + 1) * w, size=n, dtype=np.uint64))
        else:
            c = np.unique(rng.integers(lo, hi, size=n, dtype=np.uint64))
        top = (1 << 40) if big_counts else 6
        runs.append((c, rng.integers(1, top, size=c.size, dtype=np.uint64)))
    return runs


def _runs_of(rng, lens, pool=None, ones=False):
    """Runs of exactly these lengths: from one pool of codes (they overlap heavily), or, pool=None, from ranges of their
    own, the later run the lower range."""
    runs = []
    for r, n in enumerate(lens):
        if pool is None:
            lo = (len(lens) - r) << 20
            c = lo + rng.choice(3 * n + 1, size=n, replace=False)
        else:
            c = rng.choice(pool, size=n, replace=False)
        c = np.sort(c.astype(np.uint64))
        assert c.size == n and np.unique(c).size == n
        runs.append((c, np.ones(n, dtype=np.uint64) if ones else rng.integers(1, 6, size=n, dtype=np.uint64)))
    return runs


def _want(runs, min_count):
    c = np.concatenate([r[0] for r in runs])
    n = np.concatenate([r[1] for r in runs])
    u, inv = np.unique(c, return_inverse=True)
    tot = np.zeros(u.size, dtype=np.uint64)
    np.add.at(tot, inv, n)
    keep = tot >= np.uint64(min_count)
    return u[keep], tot[keep]


def _check(ctx, runs, min_count):
    run_off = np.zeros(len(runs) + 1, dtype=np.int64)
    np.cumsum([r[0].size for r in runs], out=run_off[1:])
    codes = np.concatenate([r[0] for r in runs])
    counts = np.concatenate([r[1] for r in runs])
    wc, wn = _want(runs, min_count)
    gc, gn = ctx.kmer_count_merge(run_off, codes, counts, min_count)
    assert np.array_equal(gc, wc) and np.array_equal(gn, wn)
    dc = torch.from_numpy(codes.view(np.int64)).cuda()
    dn = torch.from_numpy(counts.view(np.int64)).cuda()
    gc, gn = ctx.kmer_count_merge_dev(run_off, dc.data_ptr(), dn.data_ptr(), min_count,
                                      stream=torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(gc, wc) and np.array_equal(gn, wn)
    return wc.size


@pytest.mark.parametrize("W", [1, 2, 3, 8, 33])
def test_merge_matches_numpy(ctx, W):
    rng = np.random.default_rng(W)
    for min_count in (1, 2, 7):  # (7: only totals of several runs reach it)
        kept = _check(ctx, _runs(rng, W, 5000, hi=20000), min_count)  # (heavy overlap between runs)
        assert kept > 0 or min_count > 5 * W
    _check(ctx, _runs(rng, W, 3001, empty=(0, W - 1) if W > 1 else ()), 1)
    _check(ctx, _runs(rng, W, 4097, same=True), 2)
    _check(ctx, _runs(rng, W, 2500, disjoint=True), 1)
    # k = 31: codes up to 2^62 - 1
    _check(ctx, _runs(rng, W, 3000, lo=(1 << 62) - 50000, hi=(1 << 62)), 2)


def test_merge_counts_beyond_32_bits_and_a_threshold_only_some_reach(ctx):
    rng = np.random.default_rng(5)
    runs = _runs(rng, 4, 20000, hi=30000, big_counts=True)
    tot = _want(runs, 1)[1]
    assert int(tot.max()) > (1 << 32)
    mid = int(np.median(tot))
    n = _check(ctx, runs, mid)
    assert 0 < n < tot.size


def test_merge_large_sizes_not_multiple_of_a_tile(ctx):
    rng = np.random.default_rng(11)
    runs = []
    for r, n in enumerate((3_333_331, 2_999_999, 4_000_037)):  # ~10^7 entries
        c = np.unique(rng.integers(0, 1 << 26, size=n, dtype=np.uint64))
        runs.append((c, rng.integers(1, 4, size=c.size, dtype=np.uint64)))
    runs.append((np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)))
    assert _check(ctx, runs, 3) > 0


STRIDE_EDGE_LENS = (1, 1023, 1024, 1025, 2048, 2049, 0, 4096, 4097)  # (len - 1) // KM_STRIDE samples: 0 0 0 1 1 2 - 3 4


@pytest.mark.parametrize("min_count", [1, 2])
def test_merge_run_lengths_at_the_sample_stride(ctx, min_count):
    rng = np.random.default_rng(21)
    pool = np.unique(rng.integers(0, 1 << 40, size=5000, dtype=np.uint64))[:4500]
    assert pool.size == 4500
    kept = _check(ctx, _runs_of(rng, STRIDE_EDGE_LENS, pool=pool), min_count)
    assert 0 < kept <= 4500
    kept = _check(ctx, _runs_of(rng, STRIDE_EDGE_LENS), min_count)  # disjoint: nothing sums
    assert kept == sum(STRIDE_EDGE_LENS) if min_count == 1 else 0 < kept < sum(STRIDE_EDGE_LENS)


W_MAX = 256  # KM_MAX_RUNS: what km_tile_kernel's per-run arrays and its serial prefix are sized for


def test_merge_of_256_random_runs(ctx):
    rng = np.random.default_rng(22)
    runs = _runs(rng, W_MAX, 300, hi=2000)
    assert len(runs) == W_MAX and 200 < min(r[0].size for r in runs)
    tot = _want(runs, 1)[1]
    for min_count in (1, 2, int(np.median(tot))):
        assert _check(ctx, runs, min_count) > 0
    z = np.zeros(0, dtype=np.uint64)
    with pytest.raises(_lib.FedrannHipError, match="1 .. 256 runs"):
        ctx.kmer_count_merge(np.zeros(W_MAX + 2, dtype=np.int64), z, z, 1)  # (257 runs)


@pytest.mark.parametrize("min_count,kept", [(1, 3000), (256, 3000), (257, 0)])
def test_merge_of_256_identical_runs(ctx, min_count, kept):
    """Every code tied 256 ways, each copy counting 1: the totals are 256.  Tiles of 256 x ~1500 codes, beyond
    KM_CACHE, so the searches read global memory."""
    rng = np.random.default_rng(23)
    (codes, ones), = _runs_of(rng, [3000], ones=True)
    assert _check(ctx, [(codes, ones)] * W_MAX, min_count) == kept


@pytest.mark.parametrize("at", [0, 137, 255])
def test_merge_of_255_empty_runs_and_a_real_one(ctx, at):
    rng = np.random.default_rng(24 + at)
    lens = [0] * W_MAX
    lens[at] = 5000
    runs = _runs_of(rng, lens)
    assert _check(ctx, runs, 1) == 5000
    assert 0 < _check(ctx, runs, 3) < 5000
    assert _check(ctx, runs, 6) == 0


def test_merge_of_nothing_and_bad_arguments(ctx):
    z = np.zeros(0, dtype=np.uint64)
    gc, gn = ctx.kmer_count_merge(np.zeros(4, dtype=np.int64), z, z, 1)
    assert gc.size == 0 and gn.size == 0
    with pytest.raises(_lib.FedrannHipError):
        ctx.kmer_count_merge(np.array([1, 2], dtype=np.int64), np.ones(2, np.uint64), np.ones(2, np.uint64), 1)
    with pytest.raises(_lib.FedrannHipError):
        ctx.kmer_count_merge(np.zeros(258, dtype=np.int64), z, z, 1)  # (more than 256 runs)


def test_export_cuts_the_unthresholded_table(ctx):
    s = synth_sequences(300, genome_len=30_000, mean_len=800, k=15, seed=3)
    ctx.kmer_count_begin(15)
    ctx.kmer_count_add(s["seqs"], s["seq_off"])
    n = int(ctx.kmer_count_export_dev(0, 1)[-1])
    codes = torch.empty(n, dtype=torch.int64, device="cuda")
    counts = torch.empty(n, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ctx.kmer_count_export_dev(0, 1, codes.data_ptr(), counts.data_ptr(), stream=st)
    hc = codes.cpu().numpy().view(np.uint64)
    spl = np.sort(hc[np.random.default_rng(0).integers(0, n, size=4)]).view(np.int64)
    spl_t = torch.from_numpy(spl).cuda()
    off = ctx.kmer_count_export_dev(spl_t.data_ptr(), 5, stream=st)
    wc, wn = ctx.kmer_count_finish(1)
    assert np.array_equal(hc, wc) and np.array_equal(counts.cpu().numpy().view(np.uint64), wn)
    assert off.tolist() == [0] + np.searchsorted(wc, spl.view(np.uint64)).tolist() + [n]


def test_export_splitters_at_and_beyond_the_codes(ctx):
    """km_parts_kernel: splitters below, above and equal to codes, repeated ones, one part, and more than 256 parts
    (its second workgroup).  The table's last entry is the "no k-mer here" marker, which is not exported."""
    s = synth_sequences(200, genome_len=20_000, mean_len=600, k=15, n_rate=2e-3, seed=4)
    st = torch.cuda.current_stream().cuda_stream
    ctx.kmer_count_begin(15)
    ctx.kmer_count_add(s["seqs"], s["seq_off"])
    n = int(ctx.kmer_count_export_dev(0, 1, stream=st)[-1])
    codes = torch.empty(n, dtype=torch.int64, device="cuda")
    counts = torch.empty(n, dtype=torch.int64, device="cuda")
    assert ctx.kmer_count_export_dev(0, 1, codes.data_ptr(), counts.data_ptr(), stream=st).tolist() == [0, n]
    hc = codes.cpu().numpy().view(np.uint64)
    assert n > 1000 and hc[0] > 1 and np.all(hc[1:] > hc[:-1])
    rng = np.random.default_rng(1)
    many = np.sort(np.concatenate([rng.integers(0, int(hc[-1]) + 1000, size=279, dtype=np.uint64),
                                   hc[rng.integers(0, n, size=20)]]))
    first, mid, last, ones = int(hc[0]), int(hc[n // 2]), int(hc[-1]), (1 << 64) - 1
    sets = {
        "below the first code": [0],
        "just below the first code": [first - 1],
        "above the last code": [last + 1],
        "the marker's value": [ones],
        "the first, a middle and the last code": [first, mid, last],
        "just above a code": [int(hc[7]) + 1],
        "three equal splitters": [mid, mid, mid],
        "below and above": [0, 0, last + 1, ones],
        "299 sorted random splitters": many.tolist(),
    }
    assert many.size == 299
    for name, spl in sets.items():
        spl = np.array(spl, dtype=np.uint64)
        spl_t = torch.from_numpy(spl.view(np.int64)).cuda()
        off = ctx.kmer_count_export_dev(spl_t.data_ptr(), spl.size + 1, stream=st)
        assert off.tolist() == [0] + np.searchsorted(hc, spl, "left").tolist() + [n], name
    assert ctx.kmer_count_export_dev(0, 1, stream=st).tolist() == [0, n]  # one part
    c2 = torch.zeros(n, dtype=torch.int64, device="cuda")
    n2 = torch.zeros(n, dtype=torch.int64, device="cuda")
    spl_t = torch.from_numpy(many.view(np.int64)).cuda()
    ctx.kmer_count_export_dev(spl_t.data_ptr(), 300, c2.data_ptr(), n2.data_ptr(), stream=st)
    wc, wn = ctx.kmer_count_finish(1)
    assert wc.size == n
    for c, m in ((codes, counts), (c2, n2)):
        assert np.array_equal(c.cpu().numpy().view(np.uint64), wc) and np.array_equal(m.cpu().numpy().view(np.uint64), wn)


# ---- the CLI: sharded stage 1 against the one-GPU run ----------------------------------------------------------------
STAGE1_FILES = ["overlaps.tsv", "temp/fwd_kmer_library.fasta", "temp/rev_kmer_library.fasta",
                "temp/kmer_searcher/output.bin", "temp/kmer_searcher/kmer_frequency.bin"]
LINE = re.compile(r"rank (\d+) stage 1: bytes \[(\d+), (\d+)\), (\d+) records, (\d+) distinct k-mers owned")


def _reads(n, seed):
    s = synth_sequences(n, genome_len=60_000, mean_len=1500, k=15, seed=seed)
    return s, [bytes(s["seqs"][s["seq_off"][i]:s["seq_off"][i + 1]]) for i in range(n)]


def _fastq_bytes(ids, reads):
    return b"".join(b"@%s extra\n%s\n+\n%s\n" % (i, r, b"@" * len(r)) for i, r in zip(ids, reads))


def _run_both(tmp_path, reads_path, world, extra=()):
    base = ["-i", str(reads_path), "-k", "15", "--kmer-sample-fraction", "0.05", "-n", "128",
            "--nndescent-n-neighbors", "8", "--keep-intermediates", "--seed", "91"] + list(extra)
    one = tmp_path / "one"
    cli.main(["-o", str(one)] + base)
    many = tmp_path / "many"
    r = subprocess.run([sys.executable, "-m", "fedrann_amd", "-o", str(many), "--devices", ",".join(["0"] * world),
                        "--dist-backend", "gloo"] + base, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    files = [f for f in STAGE1_FILES if not (f.endswith("fwd_kmer_library.fasta") and "--kmer-library" in extra)]
    for f in files:
        assert (many / f).read_bytes() == (one / f).read_bytes(), f
    lines = sorted((int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in LINE.finditer(r.stderr))
    assert [x[0] for x in lines] == list(range(world)), r.stderr[-3000:]
    with open(one / "temp/kmer_searcher/output.bin", "rb") as f:
        total = struct.unpack("<4sB3sQ", f.read(16))[3]
    assert sum(x[3] for x in lines) == total
    return lines, r.stderr


def test_cli_devices_stage1_sharded_fasta(tmp_path):
    s, reads = _reads(400, 21)
    fa = tmp_path / "reads.fasta"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (i, r) for i, r in zip(s["ids"], reads)))
    lines, _ = _run_both(tmp_path, fa, 3)
    assert all(hi > lo and n > 0 for _, lo, hi, n in lines)  # every rank counted and searched a range of its own
    assert lines[0][1] == 0 and lines[-1][2] == fa.stat().st_size


def test_cli_devices_stage1_sharded_fastq(tmp_path):
    s, reads = _reads(300, 22)
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(_fastq_bytes(s["ids"], reads))  # (quality lines starting with '@')
    lines, err = _run_both(tmp_path, fq, 3)
    assert all(hi > lo for _, lo, hi, _ in lines) and "redoing stage 1" not in err


def test_cli_devices_stage1_sharded_gz(tmp_path):
    s, reads = _reads(300, 23)
    gz = tmp_path / "reads.fasta.gz"
    with gzip.open(gz, "wb") as f:
        f.write(b"".join(b">%s\n%s\n" % (i, r) for i, r in zip(s["ids"], reads)))
    _run_both(tmp_path, gz, 2)


def test_cli_devices_stage1_sharded_search_only(tmp_path):
    s, reads = _reads(300, 24)
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (i, r) for i, r in zip(s["ids"], reads)))
    lib = tmp_path / "lib.fasta"
    lib.write_bytes(b"".join(b">%d\n%s\n" % (3 + j % 9, x) for j, x in enumerate(s["fwd"])))
    lines, err = _run_both(tmp_path, fa, 3, ["--kmer-library", str(lib)])
    assert all(hi > lo for _, lo, hi, _ in lines)
    assert all(int(m.group(5)) == 0 for m in LINE.finditer(err))  # (search only: nothing counted)


def test_cli_devices_stage1_fastq_fallback(tmp_path):
    """A FASTQ whose middle cut lands on a quality line starting with '@' that, read from there on, looks like two
    records: rank 0's check fails, every rank redoes stage 1 with the whole file on rank 0, and the files are still
    the one-GPU run's."""
    s, reads = _reads(200, 25)
    recs = [b"@%s\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in zip(s["ids"], reads)]
    trap_a = b"@a\nACGT\n+\n"
    trap_b = b"@xyz\nACGT\n+\nACGT\n@r2\nACGT\n+\nIIII\n@r3\nACGT\n+\nIIII\n"
    for h in range(len(recs)):
        head, tail = b"".join(recs[:h]), b"".join(recs[h:])
        at = len(head) + len(trap_a)
        pad = 2 * at - (at + len(trap_b) + len(tail))
        if pad >= 2:
            break
    data = head + trap_a + trap_b + tail + b"x" * (pad - 1) + b"\n"  # (a stray last line: skipped by the walk)
    assert len(data) == 2 * at
    fq = tmp_path / "trap.fastq"
    fq.write_bytes(data)
    lines, err = _run_both(tmp_path, fq, 2)
    assert "redoing stage 1" in err
    assert lines[0][1:3] == (0, len(data)) and lines[1][1] == lines[1][2] == len(data)


def test_cli_devices_stage1_one_record_two_ranks(tmp_path):
    s, reads = _reads(1, 26)
    fa = tmp_path / "one.fasta"
    fa.write_bytes(b">only\n%s\n" % reads[0])
    lines, _ = _run_both(tmp_path, fa, 2, ["--kmer-min-multiplicity", "1", "--nndescent-n-neighbors", "2"])
    assert lines[1][1] == lines[1][2] and lines[1][3] == 0  # rank 1: an empty range
