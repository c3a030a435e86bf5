"""Host side of the sharded stage 1 of a `--devices` run (fedrann_amd/stage1_sharded.py), no GPU: the byte-range cuts
against the whole-file reader, the FASTQ predecessor check, the slice of the Bernoulli sample, and the count exchange
over gloo with a numpy stand-in for the merge kernel."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedrann_amd import kmer_search as ks
from fedrann_amd import stage1_sharded as s1
from fedrann_amd.count_kmers import sample_kmers


def _seq(rng, n):
    return bytes(rng.choice(list(b"ACGTN"), size=n, p=[0.24, 0.24, 0.24, 0.24, 0.04]).tolist())


def _fasta(rng, n_rec, crlf=False, junk=False, final_newline=True):
    nl = b"\r\n" if crlf else b"\n"
    out = [b"junk line before any header" + nl + nl] if junk else []
    for i in range(n_rec):
        name = b"" if i % 11 == 5 else b"r%d desc" % i  # (empty ids: the record is dropped)
        out.append(b">" + name + nl)
        for _ in range(int(rng.integers(1, 4))):
            out.append(_seq(rng, int(rng.integers(0, 90))) + nl)
        if i % 7 == 3:
            out.append(nl)  # an empty line
    data = b"".join(out)
    return data if final_newline else data.rstrip(b"\r\n")


def _fastq(rng, n_rec, crlf=False, junk=False, final_newline=True):
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n_rec):
        name = b"" if i % 13 == 6 else b"q%d x" % i
        s = _seq(rng, int(rng.integers(1, 120)))
        q = bytes(rng.choice(list(b"@+!#IJ"), size=len(s)).tolist())  # (quality lines starting with '@' and '+')
        out.append(b"@" + name + nl + s + nl + b"+" + nl + q + nl)
        if junk and i % 9 == 4:
            out.append(b"a stray line" + nl)  # (skipped alone by the walk)
    data = b"".join(out)
    return data if final_newline else data.rstrip(b"\r\n")


def _walk(path, **kw):
    ids, seqs = [], []
    for i, s, off in ks.iter_sequence_blocks(path, fastq_ids_as_fasta=True, chunk_bytes=kw.pop("chunk", 1 << 20),
                                             **kw):
        ids += i
        seqs += [bytes(s[off[j]:off[j + 1]]) for j in range(len(i))]
    return ids, seqs


CASES = [dict(), dict(crlf=True), dict(junk=True), dict(final_newline=False), dict(crlf=True, junk=True,
                                                                                    final_newline=False)]


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_ranges_concatenate_to_the_whole_file_walk(tmp_path, fmt, case):
    rng = np.random.default_rng(100 + case)
    for n_rec in (2, 60):  # (2 records: W larger than the record count)
        data = (_fasta if fmt == "fasta" else _fastq)(rng, n_rec, **CASES[case])
        path = str(tmp_path / ("reads.%s" % fmt))
        with open(path, "wb") as f:
            f.write(data)
        want = _walk(path)
        assert len(want[0]) > 0
        for W in range(1, 8):
            is_fastq, cuts = s1.cut_ranges(path, W)
            assert is_fastq == (fmt == "fastq")
            assert cuts[0] == 0 and cuts[-1] == len(data) and cuts == sorted(cuts) and len(cuts) == W + 1
            ids, seqs = [], []
            for r in range(W):
                st = {}
                i, s = _walk(path, start=cuts[r], end=cuts[r + 1], is_fastq=is_fastq, status=st, chunk=64)
                assert st["aligned"] or cuts[r + 1] == len(data), (W, r, cuts)
                ids += i
                seqs += s
            assert (ids, seqs) == want, (W, cuts)


def _trap_fastq():
    """Normal records, then a record whose quality line starts with '@' followed by lines that, read from that quality
    line on, hold the four-line pattern twice -- a wrong cut -- then more records; the quality line sits at half the
    file, where cut_ranges(W = 2) looks."""
    head = b"".join(b"@h%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i for i in range(6))
    trap_a = b"@a\nACGT\n+\n"
    trap_b = b"@xyz\nACGT\n+\nACGT\n@r2\nACGT\n+\nIIII\n@r3\nACGT\n+\nIIII\n"
    at = len(head) + len(trap_a)  # (the quality line '@xyz' of record a)
    tail_len = 2 * at - at - len(trap_b)
    tail = b""
    i = 0
    while tail_len - len(tail) > 40:
        tail += b"@t%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i
        i += 1
    rem = tail_len - len(tail)
    name = b"@z" if rem % 2 else b"@zz"  # (the last record takes 2 n + 5 + len(name) bytes)
    n = (rem - 5 - len(name)) // 2
    tail += name + b"\n" + b"C" * n + b"\n+\n" + b"I" * n + b"\n"
    data = head + trap_a + trap_b + tail
    assert len(data) == 2 * at
    return data, at


def test_wrong_fastq_cut_is_caught_by_the_predecessor_check(tmp_path):
    data, at = _trap_fastq()
    path = str(tmp_path / "trap.fastq")
    with open(path, "wb") as f:
        f.write(data)
    is_fastq, cuts = s1.cut_ranges(path, 2)
    assert is_fastq and cuts == [0, at, len(data)]  # the proposal is the quality line
    st = {}
    _walk(path, start=0, end=at, is_fastq=True, status=st)
    assert st["aligned"] is False  # rank 0's walk does not reach the cut as a record boundary
    # the fallback cuts give the whole-file walk
    whole = _walk(path)
    st = {}
    assert _walk(path, start=0, end=len(data), is_fastq=True, status=st) == whole and st["aligned"]
    # a good cut passes
    good = len(b"".join(b"@h%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i for i in range(3)))
    st = {}
    _walk(path, start=0, end=good, is_fastq=True, status=st)
    assert st["aligned"] is True


def test_format_comes_from_the_file_not_the_range(tmp_path):
    path = str(tmp_path / "r.fasta")
    with open(path, "wb") as f:
        f.write(b">a\nACGT\n@b\nACGT\n+\nIIII\n")
    # the range starting at '@b' is still FASTA: '@b' and the rest are sequence lines of nothing (no header yet)
    assert _walk(path, start=8, end=None, is_fastq=False) == ([], [])
    with pytest.raises(ValueError):
        list(ks.iter_sequence_blocks(path, start=8))


def test_sample_slice_equals_the_full_stream():
    rng = np.random.default_rng(9)
    for _ in range(40):
        N = int(rng.integers(0, 20000))
        o = int(rng.integers(0, N + 1))
        n = int(rng.integers(0, N - o + 1))
        seed, p = int(rng.integers(0, 2 ** 31)), float(rng.choice([0.005, 0.1, 0.5]))
        full = sample_kmers(N, p, seed)
        want = full[(full >= o) & (full < o + n)] - o
        assert np.array_equal(s1.sample_slice(seed, p, o, n), want)


def _np_merge(run_off, codes, counts, min_count):
    c = codes.numpy().view(np.uint64)
    n = counts.numpy().view(np.uint64)
    for r in range(run_off.size - 1):  # (each run strictly ascending)
        assert np.all(np.diff(c[run_off[r]:run_off[r + 1]].astype(np.int64)) > 0)
    u, inv = np.unique(c, return_inverse=True)
    tot = np.zeros(u.size, dtype=np.uint64)
    np.add.at(tot, inv, n)
    keep = tot >= np.uint64(min_count)
    return u[keep], tot[keep]


def _tables(world, seed):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(world):
        n = 0 if r == 1 else int(rng.integers(1, 3000))  # (rank 1: an empty table)
        c = np.unique(rng.integers(0, 1 << 14, size=n).astype(np.int64) * (1 << 47))
        out.append((c, rng.integers(1, 5, size=c.size).astype(np.int64)))
    return out


def _exchange_worker(rank, world, init, seed, min_count, outdir):
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    codes, counts = _tables(world, seed)[rank]

    def part_offsets(spl):
        assert spl.size == world - 1 and np.all(np.diff(spl) >= 0)
        return np.concatenate(([0], np.searchsorted(codes, spl), [codes.size]))

    kc, kn, o_r, N = s1.exchange_counts(torch.from_numpy(codes), torch.from_numpy(counts), min_count, part_offsets,
                                        _np_merge)
    np.savez(os.path.join(outdir, "r%d.npz" % rank), codes=kc, counts=kn, o=o_r, N=N)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("min_count", [1, 3])
def test_exchange_over_gloo_gives_the_global_table(tmp_path, world, min_count):
    init = "file://" + str(tmp_path / "rendezvous")
    mp.spawn(_exchange_worker, args=(world, init, 17 + world, min_count, str(tmp_path)), nprocs=world)
    tabs = _tables(world, 17 + world)
    allc = np.concatenate([t[0] for t in tabs])
    u, inv = np.unique(allc, return_inverse=True)
    tot = np.zeros(u.size, dtype=np.int64)
    np.add.at(tot, inv, np.concatenate([t[1] for t in tabs]))
    keep = tot >= min_count
    got = [np.load(str(tmp_path / ("r%d.npz" % r))) for r in range(world)]
    assert np.array_equal(np.concatenate([g["codes"] for g in got]).astype(np.int64), u[keep])
    assert np.array_equal(np.concatenate([g["counts"] for g in got]).astype(np.int64), tot[keep])
    offs = np.cumsum([0] + [g["codes"].size for g in got])
    assert [int(g["o"]) for g in got] == offs[:-1].tolist()
    assert all(int(g["N"]) == int(keep.sum()) for g in got)
