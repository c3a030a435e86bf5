"""Stage 1 of a `--devices` run, sharded over the ranks: k-mer counting, sampling and search of a byte range each.

The parent (no GPU) cuts the plain reads file into W byte ranges at record starts (cut_ranges) and passes the cuts
to the ranks.  Each rank then, inside the process group:

    count     its range (fdr_kmer_count_begin / _add), no threshold: min_multiplicity applies to global totals
    exchange  W - 1 splitter codes from all-gathered quantile samples of the local tables; the table is cut there
              (fdr_kmer_count_export_dev), part p goes to rank p (all_to_all_single), and the W runs received are
              merged with the threshold applied (fdr_kmer_count_merge_dev / fdr_kmer_count_merge)
    number    rank r's kept codes are the global ascending list from o_r = the kept counts of the lower ranks on;
              its share of the Bernoulli sample is the slice [o_r, o_r + n_r) of the one-GPU stream (sample_slice)
    library   the sampled k-mers are all-gathered: every rank holds the whole forward library; rank 0 writes the two
              library files
    search    its range into a records-only part file; the parts are written into one output.bin at their offsets,
              and the per-index frequencies are summed for kmer_frequency.bin

The files are byte for byte those of the one-GPU path (count_kmers.run_kmer_searcher / __main__._gpu_kmer_search):
the library is always the global ascending set, whatever the splitters, and the records keep the file order.

FASTQ cuts are proposals (the reader's walk is stateful: a quality line may start with '@'): the rank before a cut
checks that its walk reaches the cut as a record boundary, the checks are all-reduced, and if any fails every rank
redoes stage 1 with the cuts [0, B, ..., B] (rank 0 reads the whole file: same code path, same result).
"""
import logging
import os
import struct
import time
from os.path import join

import numpy as np

logger = logging.getLogger("fedrann_amd")

_PROBE = 1 << 16        # bytes read around a nominal offset at first
_PROBE_MAX = 1 << 26    # ... doubled up to this; no record start found within it: the cut moves to the end


def _fasta_cut(f, x, size):
    """First '\\n>' at or after offset x - 1: the cut is the '>' (a header resets the reader's record state)."""
    if x <= 0:
        return 0
    span = _PROBE
    while True:
        f.seek(x - 1)
        chunk = f.read(span)
        p = chunk.find(b"\n>")
        if p >= 0:
            return x + p
        if x - 1 + len(chunk) >= size or span >= _PROBE_MAX:
            return size
        span *= 2


def _two_fastq_records(lines):
    """Do lines (without their '\n') begin with two FASTQ records -- '@' header, sequence, '+' line, quality of the
    sequence's length -- or, when they end the file, with one?"""
    if len(lines) < 4:
        return False
    for r in range(0, min(len(lines), 8), 4):
        rec = lines[r:r + 4]
        if len(rec) < 4 or not (rec[0][:1] == b"@" and rec[2][:1] == b"+" and len(rec[1]) == len(rec[3])):
            return False
    return True


def _fastq_cut(f, x, size):
    """A proposed cut at or after offset x: the first line start where the four-line pattern holds for two records in
    a row (one at the end of the file).  Only a proposal: the rank before it checks it (iter_sequence_blocks status)."""
    if x <= 0:
        return 0
    span = _PROBE
    while True:
        f.seek(x - 1)
        chunk = f.read(span)
        at_end = x - 1 + len(chunk) >= size
        lines = chunk.split(b"\n")
        if not at_end or lines[-1] == b"":
            lines.pop()  # (an unterminated piece waits for more bytes; after a final '\n' there is no line)
        pos = x - 1 + len(lines[0]) + 1 if lines else size  # lines[0]: the rest of the line holding byte x - 1
        for i in range(1, len(lines)):
            if len(lines) - i < 8 and not at_end:
                break  # (more bytes needed)
            if _two_fastq_records(lines[i:i + 8]):
                return pos
            pos += len(lines[i]) + 1
        if at_end or span >= _PROBE_MAX:
            return size
        span *= 2


def cut_ranges(path, world):
    """W + 1 cuts of the plain reads file into nearly equal byte ranges at record starts, and the file's format
    (FASTQ iff its first byte is '@', as iter_sequence_blocks decides it).  Reads a few KiB around each nominal
    offset.  Ranges may be empty."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        is_fastq = f.read(1) == b"@"
        cut = _fastq_cut if is_fastq else _fasta_cut
        cuts = [0]
        for r in range(1, world):
            x = size * r // world
            cuts.append(max(cuts[-1], cut(f, x, size)) if x > cuts[-1] else cuts[-1])
        cuts.append(size)
    return is_fastq, cuts


def format_cuts(is_fastq, cuts):
    return "%s:%s" % ("fastq" if is_fastq else "fasta", ",".join(str(int(c)) for c in cuts))


def parse_cuts(text):
    fmt, _, rest = text.partition(":")
    return fmt == "fastq", [int(c) for c in rest.split(",")]


def sample_slice(seed, sample_fraction, offset, n):
    """Rank r's share of count_kmers.sample_kmers(N, p, seed): the indices i in [0, n) where draw offset + i of the
    one-GPU stream is kept.  Generator.random() takes one 64-bit output per draw, so advancing the bit generator by
    `offset` outputs lands exactly on draw `offset`."""
    bg = np.random.PCG64(int(seed))
    bg.advance(int(offset))
    return np.flatnonzero(np.random.Generator(bg).random(int(n)) > 1.0 - float(sample_fraction))


def quantile_samples(codes, n_samples=1024):
    """Up to n_samples evenly spaced codes of an ascending table (a numpy array or a torch tensor) as numpy int64."""
    n = int(codes.shape[0])
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    at = np.unique(np.linspace(0, n - 1, num=min(n, n_samples)).astype(np.int64))
    if isinstance(codes, np.ndarray):
        return codes[at].astype(np.int64)
    import torch
    return codes[torch.from_numpy(at).to(codes.device)].cpu().numpy().astype(np.int64)


def choose_splitters(samples, world):
    """W - 1 ascending splitter codes from the ranks' samples: every rank's code range then holds a similar number of
    distinct codes.  (The result of stage 1 does not depend on them; only the balance does.)"""
    allc = np.sort(np.concatenate([np.asarray(s, dtype=np.int64) for s in samples]))
    if allc.size == 0:
        return np.zeros(world - 1, dtype=np.int64)
    return allc[[min(allc.size - 1, (p + 1) * allc.size // world) for p in range(world - 1)]]


def exchange_counts(codes, counts, min_count, part_offsets, merge, group=None):
    """The global count table, sharded by code range.  codes / counts: torch int64 tensors of this rank's unthresholded
    table, ascending in code (on the device under nccl, on the host under gloo).  part_offsets(splitters) -> int64
    [W + 1]: where the table is cut (fdr_kmer_count_export_dev); merge(run_off, codes, counts, min_count) -> (codes,
    counts) numpy: the received runs merged, equal codes summed, totals >= min_count kept.  Returns (codes, counts,
    o_r, N): this rank's kept k-mers, which are the global ascending list's [o_r, o_r + n_r) of N."""
    import torch
    import torch.distributed as dist
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    samples = [None] * world
    dist.all_gather_object(samples, quantile_samples(codes), group=group)
    off = np.asarray(part_offsets(choose_splitters(samples, world)), dtype=np.int64)
    offs = [None] * world
    dist.all_gather_object(offs, off, group=group)
    send = np.diff(off).tolist()
    recv = [int(o[rank + 1] - o[rank]) for o in offs]
    n_recv = sum(recv)
    r_codes = torch.empty(n_recv, dtype=torch.int64, device=codes.device)
    r_counts = torch.empty(n_recv, dtype=torch.int64, device=codes.device)
    dist.all_to_all_single(r_codes, codes[:off[-1]].contiguous(), recv, send, group=group)
    dist.all_to_all_single(r_counts, counts[:off[-1]].contiguous(), recv, send, group=group)
    run_off = np.zeros(world + 1, dtype=np.int64)
    np.cumsum(recv, out=run_off[1:])
    kc, kn = merge(run_off, r_codes, r_counts, int(min_count))
    sizes = [None] * world
    dist.all_gather_object(sizes, int(kc.size), group=group)
    return kc, kn, int(sum(sizes[:rank])), int(sum(sizes))


def reverse_library_text(fwd_bytes):
    """rev_kmer_library.fasta from the forward one: every k-mer line reverse-complemented, the headers as they are
    (`seqkit seq -r -p`, count_kmers.py:127)."""
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    return b"\n".join(l if l.startswith(b">") else l.translate(comp)[::-1] for l in fwd_bytes.split(b"\n"))


def _all_gather_arrays(arr, group=None):
    import torch.distributed as dist
    out = [None] * dist.get_world_size(group)
    dist.all_gather_object(out, arr, group=group)
    return out


def run_stage1_rank(args, temp_dir, ctx, device, backend, cuts, is_fastq, input_path):
    """Stage 1 on this rank (see the module docstring).  Returns (path of output.bin, path of the forward library)."""
    import torch
    import torch.distributed as dist
    from . import global_variables
    from .count_kmers import revcomp_codes, write_kmer_library
    from .kmer_search import iter_sequence_blocks, read_library_files, search_append, unique_first
    rank, world = dist.get_rank(), dist.get_world_size()
    k = int(args.kmer_size)
    stream = torch.cuda.current_stream(device).cuda_stream
    on_dev = backend == "nccl"
    size = cuts[-1]

    def blocks(c, status=None):
        return iter_sequence_blocks(input_path, fastq_ids_as_fasta=True, reuse_buffers=True, start=c[rank],
                                    end=c[rank + 1], is_fastq=is_fastq, status=status)

    def cuts_hold(status, c):
        # the walk of the range before a cut must reach it as a record boundary (the last range ends at the file's end)
        ok = torch.tensor([1 if (status["aligned"] or c[rank + 1] >= size) else 0], dtype=torch.int32,
                          device=device if on_dev else "cpu")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        return bool(ok.item())

    fallback = [0] + [size] * world

    def fall_back():
        if rank == 0:
            logger.warning("stage 1: a FASTQ cut is not a record boundary of the reader's walk; redoing stage 1 with "
                           "the whole file on rank 0 (cuts %s)", fallback)
        return fallback

    t0 = time.perf_counter()
    owned = 0
    if args.kmer_library:
        fwd_path = args.kmer_library
        if rank == 0:
            with open(fwd_path, "rb") as f:
                rev_text = reverse_library_text(f.read())
            with open(join(temp_dir, "rev_kmer_library.fasta"), "wb") as f:
                f.write(rev_text)
        dist.barrier()
        lib_codes = read_library_files([fwd_path, join(temp_dir, "rev_kmer_library.fasta")], k)
    else:
        def count(c):
            status = {}
            ctx.kmer_count_begin(k)
            for _, seqs, off in blocks(c, status):
                ctx.kmer_count_add(seqs, off)
            return status

        if not cuts_hold(count(cuts), cuts):
            cuts = fall_back()
            count(cuts)
        n_local = int(ctx.kmer_count_export_dev(0, 1)[-1])
        codes_t = torch.empty(n_local, dtype=torch.int64, device=device)
        counts_t = torch.empty(n_local, dtype=torch.int64, device=device)
        ctx.kmer_count_export_dev(0, 1, codes_t.data_ptr(), counts_t.data_ptr(), stream=stream)

        def part_offsets(spl):
            spl_t = torch.from_numpy(np.ascontiguousarray(spl, dtype=np.int64)).to(device)
            return ctx.kmer_count_export_dev(spl_t.data_ptr(), world, stream=stream)

        if on_dev:
            def merge(run_off, c, n, minc):
                torch.cuda.current_stream(device).synchronize()
                return ctx.kmer_count_merge_dev(run_off, c.data_ptr(), n.data_ptr(), minc, stream=stream)
        else:
            codes_t, counts_t = codes_t.cpu(), counts_t.cpu()

            def merge(run_off, c, n, minc):
                return ctx.kmer_count_merge(run_off, c.numpy().view(np.uint64), n.numpy().view(np.uint64), minc)

        codes, counts, o_r, N = exchange_counts(codes_t, counts_t, args.kmer_min_multiplicity, part_offsets, merge)
        del codes_t, counts_t
        owned = int(codes.size)
        keep = sample_slice(global_variables.seed, args.kmer_sample_fraction, o_r, codes.size)
        parts = _all_gather_arrays((codes[keep], counts[keep]))
        fwd_codes = np.concatenate([p[0] for p in parts]).astype(np.uint64)
        fwd_counts = np.concatenate([p[1] for p in parts]).astype(np.uint64)
        rev_codes = revcomp_codes(fwd_codes, k)
        fwd_path = join(temp_dir, "fwd_kmer_library.fasta")
        if rank == 0:
            write_kmer_library(fwd_path, fwd_codes, fwd_counts, k)
            write_kmer_library(join(temp_dir, "rev_kmer_library.fasta"), rev_codes, fwd_counts, k)
        lib_codes = unique_first(np.concatenate((fwd_codes, rev_codes)))
        logger.debug("rank %d: %d of %d kept k-mers from %d on, %d sampled of %d", rank, codes.size, N, o_r, keep.size,
                     fwd_codes.size)
    t_count = time.perf_counter() - t0

    # ---- search: a records-only part file per rank, then one output.bin ----
    t0 = time.perf_counter()
    out_dir = join(temp_dir, "kmer_searcher")
    os.makedirs(out_dir, exist_ok=True)
    part = join(out_dir, "output.part%d.bin" % rank)
    final_bin = join(out_dir, "output.bin")
    tmp_bin = final_bin + ".tmp"

    def search(c, status=None):
        open(part, "wb").close()
        freq = np.zeros(int(lib_codes.size), dtype=np.int64)
        n_reads, _ = search_append(part, blocks(c, status), lib_codes, k, freq, context=ctx)
        return n_reads, freq

    if args.kmer_library:  # (no counting pass has checked the cuts)
        status = {}
        n_reads, freq = search(cuts, status)
        if not cuts_hold(status, cuts):
            cuts = fall_back()
            n_reads, freq = search(cuts)
    else:
        n_reads, freq = search(cuts)
    sizes = _all_gather_arrays((os.path.getsize(part), n_reads))
    total_bytes = sum(s for s, _ in sizes)
    total_reads = sum(n for _, n in sizes)
    if rank == 0:
        if os.path.exists(final_bin):
            os.remove(final_bin)
        with open(tmp_bin, "wb") as f:
            f.write(struct.pack("<4sB3sQ", b"KMER", 1, b"\0\0\0", total_reads))
            f.truncate(16 + total_bytes)
    dist.barrier()
    at = 16 + sum(s for s, _ in sizes[:rank])
    fd = os.open(tmp_bin, os.O_WRONLY)
    try:
        with open(part, "rb") as src:
            while True:
                chunk = src.read(1 << 24)
                if not chunk:
                    break
                os.pwrite(fd, chunk, at)
                at += len(chunk)
    finally:
        os.close(fd)
    os.remove(part)
    freq_t = torch.from_numpy(freq).to(device) if on_dev else torch.from_numpy(freq)
    dist.all_reduce(freq_t)
    dist.barrier()
    if rank == 0:
        from .kmer_search import write_frequency_counts
        os.replace(tmp_bin, final_bin)
        write_frequency_counts(join(out_dir, "kmer_frequency.bin"), freq_t.cpu().numpy())
    t_search = time.perf_counter() - t0
    logger.info("rank %d stage 1: bytes [%d, %d), %d records, %d distinct k-mers owned, count %.3f s, search %.3f s",
                rank, cuts[rank], cuts[rank + 1], n_reads, owned, t_count, t_search)
    dist.barrier()  # (output.bin and the library files are complete for every rank)
    return final_bin, fwd_path
