"""Time the radius search of the sparse index (SparseIndex.radius_search) next to the k-NN search of the same index.

    python devtools/bench_sparse_radius.py [--reads 100000 1000000] [--metrics jaccard cosine] [--hits 5 20 100]
                                           [--k 20] [--steps 3] [--block-rows 65536] [--sample 512]

Rows: synth(R, doubling=True) (2 R rows), value of feature f = idf[f] under cosine, the sets under jaccard (what
--no-projection searches; the generator of tests/test_gpu_sparse_knn.py::_synth_idf).  Per size and metric the index is
built once.  The baseline is SparseIndex.search(k) of all rows in the same row blocks (host to host: it synchronises
and copies its results out).  For each target in --hits a radius is chosen from the k = 128 lists of a sample of rows
so that the mean row has roughly that many hits (self included), and radius_search of all rows runs in the same row
blocks, host to host, the hits fetched.  One JSON line per (size, metric): "knn_ms", and per radius "radius", "hits"
(total), "hits_per_query", "longest_row", "ms", "ms_all", "ratio" = ms / knn_ms, "range_queries" (of the last block).
The radius search walks the postings twice (count, emit): the expectation from the code is a ratio of about 2, less
what the k-NN search spends on its distance-1 fill and more for the heavy queries' segmented sort and the copy of the
hits.  Kernel times alone: run it under rocprofv3 --kernel-trace --stats (sp_radius_kernel<RANGE, EMIT, METRIC>:
EMIT = false is the count pass).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.precompute import idf_weights  # noqa: E402
from fedrann_amd.synth import synth  # noqa: E402


def _timed(fn, steps):
    fn()  # warm-up: allocations, first launches
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), [round(x, 2) for x in t], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--metrics", nargs="+", choices=["cosine", "jaccard", "weighted_jaccard"], default=["jaccard", "cosine"])
    ap.add_argument("--hits", type=int, nargs="+", default=[5, 20, 100], help="mean hits per query to aim the radii at")
    ap.add_argument("--k", type=int, default=20, help="k of the baseline search")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--block-rows", type=int, default=1 << 16)
    ap.add_argument("--sample", type=int, default=512, help="rows whose k = 128 lists choose the radii")
    a = ap.parse_args()
    ctx = _lib.Context(int(os.environ.get("FEDRANN_DEVICE", "0")))
    for R in a.reads:
        s = synth(R, doubling=True)
        indptr, indices, F = s["indptr"], s["indices"], s["n_features"]
        n = indptr.size - 1
        blocks = [(lo, min(n, lo + a.block_rows)) for lo in range(0, n, a.block_rows)]
        for metric in a.metrics:
            values = None if metric == "jaccard" else idf_weights(s["counts"], F)[indices]
            if values is not None and metric == "weighted_jaccard":
                values = np.maximum(values, np.float32(0))
            with ctx.sparse_index(indptr, indices, values, F, metric=metric) as index:
                def knn():
                    for lo, hi in blocks:
                        index.search(a.k, lo, hi)
                knn_ms, knn_all, _ = _timed(knn, a.steps)
                # the radii: the distance below which the sample's lists hold `hits` entries per row
                step = max(1, n // a.sample)
                rows = np.arange(0, n, step)[:a.sample]
                d = np.sort(np.concatenate([index.search(min(128, n), int(q), int(q) + 1)[1][0] for q in rows]))
                d = d[d < 1.0]
                out = {"reads": R, "rows": n, "metric": metric, "k": a.k, "block_rows": a.block_rows,
                       "knn_ms": round(knn_ms, 2), "knn_ms_all": knn_all, "radii": []}
                for h in a.hits:
                    at = min(d.size - 1, h * rows.size)
                    radius = float(min(np.float32(d[at]), np.float32(0.999)))

                    def radius_search():
                        total, longest = 0, 0
                        for lo, hi in blocks:
                            ip, idx, dist = index.radius_search(radius, lo, hi)
                            total += int(ip[-1])
                            longest = max(longest, int(np.diff(ip).max()))
                        return total, longest
                    ms, ms_all, (total, longest) = _timed(radius_search, a.steps)
                    out["radii"].append({"aim": h, "radius": round(radius, 6), "hits": total,
                                         "hits_per_query": round(total / n, 2), "longest_row": longest,
                                         "ms": round(ms, 2), "ms_all": ms_all, "ratio": round(ms / knn_ms, 3),
                                         "range_queries": ctx.last_knn_trace()["range_queries"]})
                out["index"] = index.info()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
