"""Time the exact sparse k-NN (fdr_knn_sparse) on synthetic reads with IDF values, next to the projected search.

    python devtools/bench_sparse_knn.py [--reads 100000 1000000] [--k 20] [--steps 3] [--metric cosine|jaccard|weighted_jaccard]
                                        [--values idf|none] [--split] [--world W --rank r] [--block-rows B] [--external]

Rows: synth(R, doubling=True) (2 R rows), value of feature f = idf[f] (what --no-projection searches).  For each size
it prints one JSON line: the median wall time of the knn_sparse call (host arrays in, results out: it synchronises;
the upload of the CSR is included), sum over features of df^2 (row-pair updates), the posting bytes 8 * sum df^2 over
that time, and the median wall time of embed_knn at d = 128 on the same rows (the projected path of config 3; the
compacted CSR, as the command line passes it).  Kernel times alone: run it under rocprofv3 --kernel-trace --stats.
--metric jaccard times fdr_knn_sparse_metric on the rows' sets (values=None, 4 posting bytes per pair update);
--values none gives cosine the same rows without values (every stored entry 1), the like-for-like comparison.
--metric weighted_jaccard times fdr_knn_sparse_metric on the rows with IDF values clamped at 0, as the command line
passes them (8 posting bytes per pair update, as cosine); --values none gives it ones.
"sparse_ms_all" lists every timed call, so the spread between repetitions is visible.
--split times the two halves of that call on their own as well: "build_ms" (Context.sparse_index: the host checks, the
upload, S1, the sort and S2; each build replaces the one before and reuses its buffers, as knn_sparse does) and "search_ms" (SparseIndex.search
of every row of one index, results copied out), with "index" = SparseIndex.info() (device bytes among it).
--world W --rank r (implies the index) times the search of that rank's rows of shard_rows(n, W) alone, in query
blocks of --block-rows rows if given ("rank_search_ms", "rank_rows"): what one rank of distributed.sparse_knn_rank
searches after its build.
--external (implies the index) times SparseIndex.query of the index's OWN rows, passed as a query CSR, against
SparseIndex.search of the same rows, alternating the two calls ("ext_search_ms", "ext_query_ms", each with its _all
list): the same search kernels on the same rows with the same results, so "ext_extra_ms" = query - search is the
queries' upload, their row kernel and the run lookup, and "ext_extra_share" is that over the search.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.precompute import build_precompute_matrix, idf_weights  # noqa: E402
from fedrann_amd.synth import synth  # noqa: E402


def _median_ms(fn, steps):
    fn()  # warm-up: allocations, first launches
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), [round(x, 2) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-projected", action="store_true", help="skip the d = 128 comparison")
    ap.add_argument("--metric", choices=["cosine", "jaccard", "weighted_jaccard"], default="cosine")
    ap.add_argument("--values", choices=["idf", "none"], default="idf",
                    help="cosine, weighted_jaccard: IDF values, or none (ones)")
    ap.add_argument("--split", action="store_true", help="time the index build and the search of all rows separately too")
    ap.add_argument("--world", type=int, default=0, help="with --rank: time the search of one rank's rows of the index")
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--block-rows", type=int, default=None, help="with --world: search in query blocks of this many rows")
    ap.add_argument("--external", action="store_true",
                    help="time SparseIndex.query of the index's own rows against SparseIndex.search of them")
    a = ap.parse_args()
    ctx = _lib.Context(int(os.environ.get("FEDRANN_DEVICE", "0")))
    for R in a.reads:
        s = synth(R, doubling=True)
        indptr, indices, F = s["indptr"], s["indices"], s["n_features"]
        values = None if a.metric == "jaccard" or a.values == "none" else idf_weights(s["counts"], F)[indices]
        if values is not None and a.metric == "weighted_jaccard":
            values = np.maximum(values, np.float32(0))  # (a negative IDF carries weight 0, as on the command line)
        entry_bytes = 4 if a.metric == "jaccard" else 8
        n = indptr.size - 1
        df = np.bincount(indices, minlength=F).astype(np.float64)
        sum_df2 = float(np.sum(df * df))
        ms, all_ms = _median_ms(lambda: ctx.knn_sparse(indptr, indices, values, F, a.k, metric=a.metric), a.steps)
        trace = ctx.last_knn_trace()
        out = {"reads": R, "rows": n, "n_features": F, "nnz_per_row": indices.size / n, "mean_df": float(df[df > 0].mean()),
               "max_df": int(df.max()), "sum_df2": sum_df2, "k": a.k, "metric": a.metric,
               "values": "none" if values is None else "idf", "sparse_ms": round(ms, 2), "sparse_ms_all": all_ms,
               "posting_GBps": round(entry_bytes * sum_df2 / (ms * 1e-3) / 1e9, 1), "range_queries": trace["range_queries"],
               "zero_queries": trace["zero_queries"]}
        if a.split or a.world or a.external:
            from fedrann_amd.distributed import sparse_rank_blocks

            def build():  # (no close(): the next build replaces the index and reuses its buffers)
                ctx.sparse_index(indptr, indices, values, F, metric=a.metric)
            if a.split:
                out["build_ms"], out["build_ms_all"] = _median_ms(build, a.steps)
                out["build_ms"] = round(out["build_ms"], 2)
            with ctx.sparse_index(indptr, indices, values, F, metric=a.metric) as index:
                out["index"] = index.info()
                if a.split:
                    ms, out["search_ms_all"] = _median_ms(lambda: index.search(a.k), a.steps)
                    out["search_ms"] = round(ms, 2)
                if a.external:
                    t_search, t_query = [], []
                    index.search(a.k)  # warm-up: allocations, first launches
                    index.query(indptr, indices, values, a.k)
                    for _ in range(a.steps):
                        t0 = time.perf_counter()
                        want = index.search(a.k)
                        t1 = time.perf_counter()
                        got = index.query(indptr, indices, values, a.k)
                        t2 = time.perf_counter()
                        t_search.append((t1 - t0) * 1e3)
                        t_query.append((t2 - t1) * 1e3)
                    if not (np.array_equal(got[0], want[0]) and
                            np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))):
                        raise SystemExit("query of the index's own rows differs from the search of them")
                    sm, qm = float(np.median(t_search)), float(np.median(t_query))
                    out.update(ext_search_ms=round(sm, 2), ext_search_ms_all=[round(x, 2) for x in t_search],
                               ext_query_ms=round(qm, 2), ext_query_ms_all=[round(x, 2) for x in t_query],
                               ext_extra_ms=round(qm - sm, 2), ext_extra_share=round((qm - sm) / sm, 4),
                               index_after_query=index.info())
                if a.world:
                    lo, hi, blocks = sparse_rank_blocks(n, a.rank, a.world, a.block_rows)
                    res = (np.empty((hi - lo, a.k), np.int32), np.empty((hi - lo, a.k), np.float32))

                    def rank_search():
                        for b0, b1 in blocks:
                            index.search(a.k, b0, b1, out=(res[0][b0 - lo:b1 - lo], res[1][b0 - lo:b1 - lo]))
                    ms, out["rank_search_ms_all"] = _median_ms(rank_search, a.steps)
                    out.update(rank_search_ms=round(ms, 2), rank_rows=[lo, hi], world=a.world, rank=a.rank,
                               block_rows=a.block_rows)
        if not a.no_projected:
            P = build_precompute_matrix(s["counts"], 128, n_features=F)
            ctx.projection_load(P.indptr, P.indices, P.data, F, 128)
            cip, cix = ctx.csr_compact(indptr, indices)
            out["projected_d128_ms"] = round(_median_ms(lambda: ctx.embed_knn(cip, cix, a.k), a.steps)[0], 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
