"""Time the exact re-score of projected neighbour lists (fdr_sparse_rescore) on synthetic reads, next to the projected
search it follows and the exact sparse search it approximates, and measure what it does to recall.

    python devtools/bench_rescore.py [--reads 100000 1000000] [--k 20] [--candidates 40] [--steps 5]
                                     [--metrics cosine jaccard weighted_jaccard] [--dim 128]

Rows: synth(R, doubling=True) (2 R rows); the values of a metric are those of --no-projection under it (IDF weights,
clamped at 0 for weighted_jaccard, none for jaccard).  For each size and metric it prints one JSON line:
  projected_k_ms      embed_knn at k on the compacted CSR (the plain projected search)
  projected_kp_ms     embed_knn at K' (what the re-score needs in its place)
  rescore_ms          sparse_rescore of those lists, host arrays in, results out: it synchronises, and the upload of
                      the CSR is included ("upload_bytes" says how much that is)
  two_stage_ms        projected_kp_ms + rescore_ms
  sparse_ms           knn_sparse at k under the same metric on the same rows: the exact search
  recall_projected    recall@k of the plain projected lists against the exact lists
  recall_rescored     recall@k of the re-scored lists against the exact lists
  pair_entries        sum over the (query, candidate) pairs of the candidate's stored entries: what the kernel streams
Every time is the median of --steps calls after one warm-up call; the *_all lists hold every timed call.  Recall counts,
per query, the indices the two lists share (an exact list's distance-1 fill and its ties at the k-th place count as any
other entry), over k.  Kernel times alone: run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.__main__ import sparse_weights  # noqa: E402
from fedrann_amd.precompute import build_precompute_matrix  # noqa: E402
from fedrann_amd.synth import synth  # noqa: E402


def _median_ms(fn, steps):
    fn()  # warm-up: allocations, first launches
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 2), [round(x, 2) for x in t]


def recall(got, want, block=1 << 16):
    """The mean over the rows of |got[q] & want[q]| / k (indices; both [n, k])."""
    n, k = want.shape
    shared = 0
    for lo in range(0, n, block):
        g, w = got[lo:lo + block], want[lo:lo + block]
        shared += int((g[:, :, None] == w[:, None, :]).any(axis=2).sum())
    return shared / (n * k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--candidates", type=int, default=40, help="K': candidates per read taken from the projected search")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--metrics", nargs="+", default=["cosine", "jaccard", "weighted_jaccard"],
                    choices=["cosine", "jaccard", "weighted_jaccard"])
    a = ap.parse_args()
    ctx = _lib.Context(int(os.environ.get("FEDRANN_DEVICE", "0")))
    for R in a.reads:
        s = synth(R, doubling=True)
        indptr, indices, F = s["indptr"], s["indices"], s["n_features"]
        n = indptr.size - 1
        P = build_precompute_matrix(s["counts"], a.dim, n_features=F)
        ctx.projection_load(P.indptr, P.indices, P.data, F, a.dim)
        cip, cix = ctx.csr_compact(indptr, indices)
        k_ms, k_all = _median_ms(lambda: ctx.embed_knn(cip, cix, a.k), a.steps)
        kp_ms, kp_all = _median_ms(lambda: ctx.embed_knn(cip, cix, a.candidates), a.steps)
        plain = ctx.embed_knn(cip, cix, a.k)[0]
        cand = ctx.embed_knn(cip, cix, a.candidates)[0]
        pair_entries = int(np.diff(indptr)[cand].sum())
        for metric in a.metrics:
            w = sparse_weights(s["counts"], F, metric)
            values = None if w is None else w[indices]
            res = (np.empty((n, a.k), np.int32), np.empty((n, a.k), np.float32))
            r_ms, r_all = _median_ms(lambda: ctx.sparse_rescore(indptr, indices, values, F, cand, k=a.k, metric=metric,
                                                                out=res), a.steps)
            s_ms, s_all = _median_ms(lambda: ctx.knn_sparse(indptr, indices, values, F, a.k, metric=metric), a.steps)
            exact = ctx.knn_sparse(indptr, indices, values, F, a.k, metric=metric)[0]
            upload = indptr.nbytes + indices.nbytes + (0 if values is None else values.nbytes) + cand.nbytes
            print(json.dumps({
                "reads": R, "rows": n, "n_features": F, "nnz_per_row": round(indices.size / n, 1), "dim": a.dim, "k": a.k,
                "candidates": a.candidates, "metric": metric, "projected_k_ms": k_ms, "projected_k_ms_all": k_all,
                "projected_kp_ms": kp_ms, "projected_kp_ms_all": kp_all, "rescore_ms": r_ms, "rescore_ms_all": r_all,
                "two_stage_ms": round(kp_ms + r_ms, 2), "sparse_ms": s_ms, "sparse_ms_all": s_all,
                "upload_bytes": upload, "pair_entries": pair_entries,
                "recall_projected": round(recall(plain, exact), 4), "recall_rescored": round(recall(res[0], exact), 4),
            }), flush=True)


if __name__ == "__main__":
    main()
