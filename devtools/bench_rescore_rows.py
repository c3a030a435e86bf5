"""Time the held re-score rows (fdr_rescore_rows_*) on synthetic reads: the build, the rectangular call on held rows
next to fdr_sparse_rescore on the same lists, and the ragged re-score of projected radius rows, in blocks as the command
line runs it; measure what the re-scored radius rows recall of the exact radius search.

    python devtools/bench_rescore_rows.py [--reads 100000 1000000] [--candidates 40] [--per-read 20 100] [--steps 5]
                                          [--metrics cosine jaccard weighted_jaccard] [--dim 128] [--long-row 20000]
                                          [--recall-reads 100000] [--only knn|radius|long] [--block-rows 65536]
                                          [--drop-empty]

Rows: synth(R, doubling=True) (2 R rows); the values of a metric are those of --no-projection under it.  One process
per run, every size in it; for each size and metric it prints JSON lines:
  "what": "knn"     build_ms (one call: upload + row pass), held_knn_ms (RescoreRows.knn at K' = --candidates) and
                    rescore_ms (Context.sparse_rescore of the same lists: the path that uploads the CSR per call), their
                    difference, upload_bytes, pair_entries (sum over the pairs of the candidate's stored entries)
  "what": "radius"  per --per-read target P: the projected radius R whose rows hold about P candidates per read (found
                    by bisection on a sample of rows), dense_ms (DenseIndex.radius_search of all rows in blocks),
                    ragged_ms at R2 = 1 and at the R2 that keeps about half (the median exact distance; where that is 1,
                    the largest distance below 1) (RescoreRows.radius of those rows, host arrays in, results out, in the
                    same blocks), candidates, hits, pair_entries, and at --recall-reads
                    the recall of the re-scored rows against SparseIndex.radius_search(R2)
  "what": "long"    one call of short rows with and without a single row of --long-row candidates
Every time is the median of --steps calls after one warm-up call; the *_all lists hold every timed call.  Kernel times
alone: run it under rocprofv3 --kernel-trace --stats with --only radius (X3 is sparse_rescore_ragged_kernel, X2
sparse_rescore_kernel; the sort is rocprim's segmented_radix_sort kernels, the split radius_split_kernel).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.__main__ import RADIUS_BLOCK_ROWS, RADIUS_MAX_HITS, sparse_weights  # noqa: E402
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


BLOCK_ROWS = RADIUS_BLOCK_ROWS  # --block-rows


def _blocks(n):
    return [(lo, min(n, lo + BLOCK_ROWS)) for lo in range(0, n, BLOCK_ROWS)]


def _radius_for(dense, n, per_read, sample=2048):
    """the projected radius at which a sample of rows holds about per_read candidates each (bisection)"""
    lo_r, hi_r = 0.0, 0.999
    a = max(0, n // 2 - sample // 2)
    b = min(n, a + sample)
    for _ in range(18):
        mid = (lo_r + hi_r) / 2
        got = dense.radius_search(mid, a, b, max_hits=RADIUS_MAX_HITS)[0][-1] / (b - a)
        if got < per_read:
            lo_r = mid
        else:
            hi_r = mid
    return round(hi_r, 5)


def _recall(got, want):
    """the share of the exact rows' entries that the re-scored rows hold (rows as (indptr, idx))"""
    shared = total = 0
    for q in range(want[0].size - 1):
        w = want[1][want[0][q]:want[0][q + 1]]
        g = got[1][got[0][q]:got[0][q + 1]]
        shared += np.intersect1d(w, g).size
        total += w.size
    return shared / max(total, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--candidates", type=int, default=40, help="K' of the rectangular comparison")
    ap.add_argument("--per-read", type=int, nargs="+", default=[20, 100], help="candidates per read of the radius runs")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--long-row", type=int, default=20000)
    ap.add_argument("--recall-reads", type=int, default=100_000)
    ap.add_argument("--block-rows", type=int, default=RADIUS_BLOCK_ROWS, help="query rows per radius call")
    ap.add_argument("--drop-empty", action="store_true",
                    help="leave out the rows whose embedding is zero (none of their features has an entry in the projection)")
    ap.add_argument("--only", choices=["knn", "radius", "long"], default=None)
    ap.add_argument("--metrics", nargs="+", default=["cosine", "jaccard", "weighted_jaccard"],
                    choices=["cosine", "jaccard", "weighted_jaccard"])
    a = ap.parse_args()
    global BLOCK_ROWS
    BLOCK_ROWS = a.block_rows
    ctx = _lib.Context(int(os.environ.get("FEDRANN_DEVICE", "0")))
    for R in a.reads:
        s = synth(R, doubling=True)
        indptr, indices, F = s["indptr"], s["indices"], s["n_features"]
        if a.drop_empty:  # the rows the projection sees nothing of: they are all within any radius of each other
            P0 = build_precompute_matrix(s["counts"], a.dim, n_features=F)
            ctx.projection_load(P0.indptr, P0.indices, P0.data, F, a.dim)
            keep = np.diff(ctx.csr_compact(indptr, indices)[0]) > 0
            lens0 = np.diff(indptr)
            indices = np.ascontiguousarray(indices[np.repeat(keep, lens0)])
            indptr = np.zeros(int(keep.sum()) + 1, np.int64)
            np.cumsum(lens0[keep], out=indptr[1:])
        n = indptr.size - 1
        lens = np.diff(indptr)
        base = {"reads": R, "rows": n, "n_features": F, "nnz_per_row": round(indices.size / n, 1), "dim": a.dim}
        P = build_precompute_matrix(s["counts"], a.dim, n_features=F)
        ctx.projection_load(P.indptr, P.indices, P.data, F, a.dim)
        cip, cix = ctx.csr_compact(indptr, indices)
        cand = ctx.embed_knn(cip, cix, a.candidates)[0] if a.only in (None, "knn") else None
        dense = ctx.dense_index_from_csr(cip, cix) if a.only in (None, "radius") else None
        radii = {}
        if dense is not None:
            for p in a.per_read:
                r = _radius_for(dense, n, p)
                d_ms, d_all = _median_ms(lambda: [dense.radius_search(r, lo, hi, max_hits=RADIUS_MAX_HITS)
                                                  for lo, hi in _blocks(n)], a.steps)
                rows = [dense.radius_search(r, lo, hi, max_hits=RADIUS_MAX_HITS)[:2] for lo, hi in _blocks(n)]
                radii[p] = (r, d_ms, d_all, rows)
        for metric in a.metrics:
            w = sparse_weights(s["counts"], F, metric)
            values = None if w is None else w[indices]
            t0 = time.perf_counter()
            held = ctx.rescore_rows(indptr, indices, values, F, metric=metric)
            build_ms = round((time.perf_counter() - t0) * 1e3, 2)
            out = dict(base, metric=metric, build_ms=build_ms, device_bytes=held.info()["device_bytes"])
            if a.only in (None, "knn"):
                k = a.candidates
                res = (np.empty((n, k), np.int32), np.empty((n, k), np.float32))
                h_ms, h_all = _median_ms(lambda: held.knn(cand, out=res), a.steps)
                r_ms, r_all = _median_ms(lambda: ctx.sparse_rescore(indptr, indices, values, F, cand, metric=metric,
                                                                    out=res), a.steps)
                upload = indptr.nbytes + indices.nbytes + (0 if values is None else values.nbytes)
                print(json.dumps(dict(out, what="knn", candidates=k, held_knn_ms=h_ms, held_knn_ms_all=h_all,
                                      rescore_ms=r_ms, rescore_ms_all=r_all, saved_ms=round(r_ms - h_ms, 2),
                                      upload_bytes=upload, pair_entries=int(lens[cand].sum()))), flush=True)
            for p, (r, d_ms, d_all, rows) in radii.items():
                total = sum(int(ip[-1]) for ip, _ in rows)
                entries = sum(int(lens[ix].sum()) for _, ix in rows)

                def run(r2):
                    return [held.radius(ip, ix, r2, q_lo=lo, max_entries=RADIUS_MAX_HITS)
                            for (ip, ix), (lo, _) in zip(rows, _blocks(n))]
                all_ = run(1.0)
                d = np.concatenate([o[2] for o in all_])
                half = float(np.median(d)) if d.size else 1.0
                if half >= 1.0 and (d < 1).any():  # (more than half share nothing: cut exactly those)
                    half = float(d[d < 1].max())
                line = dict(out, what="radius", per_read=p, radius=r, dense_ms=d_ms, dense_ms_all=d_all, blocks=len(rows),
                            candidates=total, candidates_per_row=round(total / n, 1), pair_entries=entries)
                for name, r2 in (("all", 1.0), ("half", half)):
                    ms, ms_all = _median_ms(lambda: run(r2), a.steps)
                    hits = sum(int(o[0][-1]) for o in run(r2))
                    line.update({"r2_" + name: round(r2, 6), "ragged_%s_ms" % name: ms, "ragged_%s_ms_all" % name: ms_all,
                                 "hits_" + name: hits})
                if R <= a.recall_reads and half < 1.0:
                    got = run(half)
                    with ctx.sparse_index(indptr, indices, values, F, metric=metric) as exact:
                        shared = want_total = 0
                        for o, (lo, hi) in zip(got, _blocks(n)):
                            e = exact.radius_search(half, lo, hi, max_hits=RADIUS_MAX_HITS)
                            want_total += int(e[0][-1])
                            shared += _recall(o, e) * int(e[0][-1])
                    line.update(exact_hits=want_total, recall=round(shared / max(want_total, 1), 4))
                print(json.dumps(line), flush=True)
            if a.only in (None, "long"):
                rng = np.random.default_rng(1)
                nq = min(n, 4096)
                short = [rng.integers(0, n, 20, dtype=np.int32) for _ in range(nq)]
                long_ = list(short)
                long_[nq // 2] = rng.integers(0, n, a.long_row, dtype=np.int32)
                line = dict(out, what="long", queries=nq, long_row=a.long_row)
                for name, lists in (("short", short), ("with_long", long_)):
                    ip = np.zeros(nq + 1, np.int64)
                    np.cumsum([c.size for c in lists], out=ip[1:])
                    ix = np.concatenate(lists)
                    ms, ms_all = _median_ms(lambda: held.radius(ip, ix, 1.0), a.steps)
                    line.update({name + "_ms": ms, name + "_ms_all": ms_all})
                print(json.dumps(line), flush=True)
            held.close()
        if dense is not None:
            dense.close()


if __name__ == "__main__":
    main()
