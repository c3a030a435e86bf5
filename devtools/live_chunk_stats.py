"""Development: how many 16-component chunks are live per query block of the d <= 128 candidate pass?

    python devtools/live_chunk_stats.py [reads ...]        (default 100000 1000000)

Embeds and normalises the benchmark's rows with the CPU oracle, drops duplicate rows as the class layer does (the
pass searches unique rows; the first row of a class stands for it), orders the rest as row_chunk_keys_kernel + the
stable radix sort do -- (non-empty chunks << 32) | chunk mask -- and, for blocks of 256 consecutive rows (one
eight-wave workgroup's queries), prints the histogram of NL = chunks non-empty in at least one row of the block and
the k-step share sum(NL) / (8 * blocks): the fraction of today's MFMA k-steps a pass would issue that skips the
chunks empty in EVERY query of its block.  The same for a finer ordering (mask first, then count) and, as the floor
no ordering of whole blocks can beat, for 32-row blocks (one wave's queries).  docs/experiments.md A-22.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedrann_amd.precompute import build_precompute_matrix  # noqa: E402
from fedrann_amd.synth import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

D, CHUNK = 128, 16
NC = D // CHUNK


def chunk_masks(Eh):
    """bit c set <=> some component of chunk c is non-zero (-0.0 counts as zero, as in row_chunk_keys_kernel)"""
    nz = (Eh != 0).reshape(Eh.shape[0], NC, CHUNK).any(2)
    return (nz * (1 << np.arange(NC))).sum(1).astype(np.int64)


def popcount(m):
    return np.unpackbits(m.astype(np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def block_stats(masks, block):
    """NL of every block of `block` consecutive masks (the last block may be short)"""
    n = masks.size
    pad = (-n) % block
    m = np.concatenate([masks, np.zeros(pad, dtype=np.int64)]).reshape(-1, block)
    return popcount(np.bitwise_or.reduce(m, axis=1)), np.array([np.unique(r).size for r in m[: min(len(m), 4096)]])


def report(label, masks, block):
    nl, distinct = block_stats(masks, block)
    hist = np.bincount(nl, minlength=NC + 1)
    print("  %-44s blocks %6d  NL histogram 0..8: %s  k-step share %.3f  (distinct masks per block, first 4096 blocks: "
          "median %d, max %d)" % (label, nl.size, " ".join("%d" % h for h in hist), nl.sum() / (NC * nl.size),
                                  int(np.median(distinct)), int(distinct.max())))


def main():
    for R in [int(a) for a in sys.argv[1:]] or [100_000, 1_000_000]:
        t0 = time.time()
        s = synth(R, seed=602)
        P = build_precompute_matrix(s["counts"], D)
        E = O.embed(s["indptr"], s["indices"], (P.indptr, P.indices, P.data), s["n_features"], D)
        del s
        Eh, _, zero = O.normalize(E)
        del E
        v = np.ascontiguousarray(Eh).view(np.dtype((np.void, 4 * D))).ravel()
        _, first = np.unique(v, return_index=True)
        first.sort()  # the unique rows in row order
        print("reads %d: %d unique rows (%.1f %%), %d all-zero rows, non-zero components per row: mean %.2f  (%.0f s)"
              % (R, first.size, 100.0 * first.size / R, int(zero.sum()), (Eh != 0).sum(1).mean(), time.time() - t0))
        for what, rows in (("every row", np.arange(R)), ("unique rows (what the pass searches)", first)):
            m = chunk_masks(Eh[rows])
            cnt = popcount(m)
            print(" %s: non-empty chunks per row 0..8: %s  mean %.2f" % (what, " ".join(
                "%d" % h for h in np.bincount(cnt, minlength=NC + 1)), cnt.mean()))
            shipped = np.argsort((cnt << 32) | m, kind="stable")
            finer = np.argsort((m << 32) | cnt, kind="stable")
            report("unordered, 256-row blocks", m, 256)
            report("shipped key (count, mask), 256-row blocks", m[shipped], 256)
            report("mask first, then count, 256-row blocks", m[finer], 256)
            report("shipped key, 32-row blocks (one wave)", m[shipped], 32)


if __name__ == "__main__":
    main()
