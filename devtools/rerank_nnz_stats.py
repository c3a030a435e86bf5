"""Development: how many non-zero components does a row of the d = 128 k-NN search hold?

    python devtools/rerank_nnz_stats.py [reads ...]        (default 1000000 100000; rows sampled: the first 100 000 reads)

Embeds the benchmark's rows with the CPU oracle and prints, for the rows and for the unique rows (what the re-rank's
targets are with the duplicate-row layer on), the distribution of non-zeros per row (-0.0 counts as zero, as in
to_half_compact_kernel) and the share of rows beyond the entry counts a compact record can hold: 12 (one 64-byte
half), 16, 24 (both halves), 32.  docs/experiments.md A-32.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedrann_amd.precompute import build_precompute_matrix  # noqa: E402
from fedrann_amd.synth import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

D, SAMPLE = 128, 100_000


def report(label, nnz):
    print("  %-12s rows %7d  mean %.2f  median %d  p90 %d  p99 %d  max %d   more than 12: %.2f %%  16: %.2f %%  "
          "24: %.2f %%  32: %.3f %%" % (label, nnz.size, nnz.mean(), np.median(nnz), np.percentile(nnz, 90),
                                        np.percentile(nnz, 99), nnz.max(), *(100.0 * (nnz > c).mean() for c in (12, 16, 24, 32))))


def main():
    for R in [int(a) for a in sys.argv[1:]] or [1_000_000, 100_000]:
        s = synth(R, seed=602)
        P = build_precompute_matrix(s["counts"], D)
        n = min(R, SAMPLE)
        E = O.embed(s["indptr"][:n + 1], s["indices"][:s["indptr"][n]], (P.indptr, P.indices, P.data), s["n_features"], D)
        nnz = (E != 0).sum(1)
        v = np.ascontiguousarray(O.normalize(E)[0]).view(np.dtype((np.void, 4 * D))).ravel()
        _, first = np.unique(v, return_index=True)
        print("reads %d (rows 0 .. %d):" % (R, n))
        report("every row", nnz)
        report("unique rows", nnz[first])


if __name__ == "__main__":
    main()
