"""Time the refinement of projected neighbour lists among the neighbours of their neighbours (fdr_graph_expand +
fdr_rescore_rows_refine) on synthetic reads, next to the plain --rescore it competes with, and measure what each does to
recall against the exact lists of the same metric.

    python devtools/bench_refine.py [--reads 100000 1000000] [--k 20] [--steps 5] [--dim 128]
                                    [--metrics cosine jaccard weighted_jaccard] [--no-exact]

Rows: synth(R, doubling=True) (2 R rows); the values of a metric are those of --no-projection under it.  For each size
and metric it prints one JSON line; every time is host to host, the median of --steps calls after one warm-up call, with
every timed call in the *_all list beside it:
  projected_k_ms / projected_2k_ms   embed_knn at k and at 2 k on the compacted CSR
  rescore_k_ms / rescore_2k_ms       sparse_rescore of those lists at K' = k and K' = 2 k (the CSR's upload included):
                                     with the search in front, --rescore as the parent commit runs it (two_stage_*_ms)
  rows_build_ms                      rescore_rows: the feature rows to the device, once for all rounds
  expand_ms                          fdr_graph_expand alone over all rows (block by block, nothing fetched)
  refine1_ms / refine2_ms            one and two rounds of RescoreRows.refine at k from the projected lists at k
  refine1_reverse_ms / refine2_...   the same with reverse=True (the union graph first)
  bound / distinct                   the expansion's upper-bound entries and its distinct entries, round 1
  recall_*                           recall@k against knn_sparse at k under the metric (--no-exact: left out)
Kernel times alone: run it under rocprofv3 --kernel-trace --stats with --steps 1.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedrann_amd import _lib  # noqa: E402
from fedrann_amd import graph as fgraph  # noqa: E402
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


def recall(graph, want):
    """|row q of graph & want[q]| summed over the rows, over n k; graph rectangular idx [n, k] or ragged (indptr, idx, _)."""
    n, k = want.shape
    if isinstance(graph, np.ndarray):
        rows, idx = np.repeat(np.arange(n, dtype=np.int64), graph.shape[1]), graph.reshape(-1).astype(np.int64)
    else:
        rows, idx = np.repeat(np.arange(n, dtype=np.int64), np.diff(graph[0])), graph[1].astype(np.int64)
    got = np.unique(rows * n + idx)
    exact = np.unique(np.repeat(np.arange(n, dtype=np.int64), k) * n + want.reshape(-1))
    return np.intersect1d(got, exact, assume_unique=True).size / (n * k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--metrics", nargs="+", default=["cosine", "jaccard", "weighted_jaccard"],
                    choices=["cosine", "jaccard", "weighted_jaccard"])
    ap.add_argument("--no-exact", action="store_true", help="skip the exact search and the recalls")
    a = ap.parse_args()
    k = a.k
    ctx = _lib.Context(int(os.environ.get("FEDRANN_DEVICE", "0")))
    for R in a.reads:
        print("synth(%d) ..." % R, file=sys.stderr, flush=True)
        s = synth(R, doubling=True)
        indptr, indices, F = s["indptr"], s["indices"], s["n_features"]
        n = indptr.size - 1
        P = build_precompute_matrix(s["counts"], a.dim, n_features=F)
        ctx.projection_load(P.indptr, P.indices, P.data, F, a.dim)
        cip, cix = ctx.csr_compact(indptr, indices)
        pk_ms, pk_all = _median_ms(lambda: ctx.embed_knn(cip, cix, k), a.steps)
        p2_ms, p2_all = _median_ms(lambda: ctx.embed_knn(cip, cix, 2 * k), a.steps)
        plain = ctx.embed_knn(cip, cix, k)
        wide = ctx.embed_knn(cip, cix, 2 * k)[0]
        for metric in a.metrics:
            print("%d reads, %s ..." % (R, metric), file=sys.stderr, flush=True)
            w = sparse_weights(s["counts"], F, metric)
            values = None if w is None else w[indices]
            out = {"reads": R, "rows": n, "n_features": F, "nnz_per_row": round(indices.size / n, 1), "dim": a.dim, "k": k,
                   "metric": metric, "projected_k_ms": pk_ms, "projected_k_ms_all": pk_all, "projected_2k_ms": p2_ms,
                   "projected_2k_ms_all": p2_all}
            res = (np.empty((n, k), np.int32), np.empty((n, k), np.float32))
            lists = {}
            for name, cand in (("k", plain[0]), ("2k", wide)):
                ms, every = _median_ms(lambda: ctx.sparse_rescore(indptr, indices, values, F, cand, k=k, metric=metric,
                                                                  out=res), a.steps)
                out["rescore_%s_ms" % name], out["rescore_%s_ms_all" % name] = ms, every
                out["two_stage_%s_ms" % name] = round((pk_ms if name == "k" else p2_ms) + ms, 2)
                lists["rescored_" + name] = res[0].copy()
            t0 = time.perf_counter()
            held = ctx.rescore_rows(indptr, indices, values, F, metric=metric)
            out["rows_build_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            with held:
                gip, gix, gds = fgraph.as_ragged(plain)
                pieces = _lib.expand_pieces(fgraph.expand_bound(gip, k), 1 << 27)
                out["blocks"] = len(pieces)

                def expand_all():
                    return sum(int(ctx._graph_expand_held(n, gip, gix, gds, k, lo, hi, 1 << 27)[-1]) for lo, hi in pieces)
                out["expand_ms"], out["expand_ms_all"] = _median_ms(expand_all, a.steps)
                out["distinct"] = expand_all()
                fl = np.minimum(np.diff(gip), k)
                out["bound"] = int(fl.sum() + fl[gix].sum())  # (rows of k entries and a fan of k: every entry is followed)

                def rounds(count, reverse):
                    g = plain
                    for _ in range(count):
                        g = held.refine(g, k, reverse=reverse)
                    return g
                for name, count, reverse in (("refine1", 1, False), ("refine2", 2, False), ("refine1_reverse", 1, True),
                                             ("refine2_reverse", 2, True)):
                    out[name + "_ms"], out[name + "_ms_all"] = _median_ms(lambda: rounds(count, reverse), a.steps)
                    lists[name] = rounds(count, reverse)
                out["expand_share_of_refine1"] = round(out["expand_ms"] / out["refine1_ms"], 3)
            ctx.graph_free()
            if not a.no_exact:
                t0 = time.perf_counter()
                exact = ctx.knn_sparse(indptr, indices, values, F, k, metric=metric)[0]
                out["sparse_ms_once"] = round((time.perf_counter() - t0) * 1e3, 2)
                exact = exact.astype(np.int64)
                out["recall_projected"] = round(recall(plain[0], exact), 4)
                for name, g in lists.items():
                    out["recall_" + name] = round(recall(g, exact), 4)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
