"""Time the radius search of the dense index (DenseIndex.radius_search) next to embed_knn at k = 20 on the same rows.

    python devtools/bench_dense_radius.py [--reads 100000 1000000] [--dim 128] [--hits 5 20] [--k 20] [--steps 3]
                                          [--block-rows 65536] [--sample 512] [--baseline-tree PATH]

Rows: synth(R) embedded with the projection of its counts at d = --dim (what the default, projected mode searches).
Per size the index is built once (dense_index_from_csr on the compacted CSR).  For each target in --hits a radius is
chosen from the k = 128 lists of a sample of rows so that the mean row has roughly that many hits (self included), and
radius_search of all rows runs in row blocks, host to host, the hits fetched.  "device_ms" is the sum of the timed
spans of the same calls (fdr_timing: the two range scans under knn_prefilter, the exact pass, scans, sort and split
under knn_rerank) and "scan_ms" the range scans alone.  "cand_per_hit" is candidates / hits from fdr_dense_index_info,
summed over the blocks; "hits_between_zero_rows" of them are the closed form of the zero queries (zero_rows squared,
at every radius), which no scan produces.  The baseline is embed_knn(k) of the same compacted CSR, host to host, with "knn_pass_ms" its
fp16 candidate pass; --baseline-tree PATH measures it in a fresh child process on another built checkout (the parent
commit's, for the figures in DESIGN.md section 5) and reports it as "baseline".  One JSON line per size.
The model: two fp16 scans plus a tail proportional to the candidates, so about twice the k = 20 candidate pass.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

# (the child of --baseline-tree imports the package of that tree, whose bindings match its library)
sys.path.insert(0, os.environ.get("FEDRANN_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.precompute import build_precompute_matrix  # noqa: E402
from fedrann_amd.synth import synth  # noqa: E402

K_PREFILTER, K_RERANK = _lib.KERNELS.index("knn_prefilter"), _lib.KERNELS.index("knn_rerank")


def _timed(ctx, fn, steps):
    fn()  # warm-up: allocations, first launches
    t, spans, res = [], [], None
    ctx.timing(True)
    for _ in range(steps):
        t0 = time.perf_counter()
        res = fn()
        t.append((time.perf_counter() - t0) * 1e3)
        spans.append((ctx.timing_read(K_PREFILTER)[1], ctx.timing_read(K_RERANK)[1]))
    ctx.timing(False)
    i = int(np.argsort(t)[len(t) // 2])
    return t[i], [round(x, 2) for x in t], spans[i], res


def _rows(ctx, R, d):
    s = synth(R)
    P = build_precompute_matrix(s["counts"], d)
    ctx.projection_load(P.indptr, P.indices, P.data, s["n_features"], d)
    return ctx.csr_compact(s["indptr"], s["indices"])


def _knn(ctx, cip, cix, k, steps):
    ms, ms_all, (pass_ms, rest_ms), _ = _timed(ctx, lambda: ctx.embed_knn(cip, cix, k), steps)
    return {"k": k, "ms": round(ms, 2), "ms_all": ms_all, "knn_pass_ms": round(pass_ms, 2), "knn_rest_ms": round(rest_ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--hits", type=int, nargs="+", default=[5, 20], help="mean hits per query to aim the radii at")
    ap.add_argument("--k", type=int, default=20, help="k of the baseline search")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--block-rows", type=int, default=1 << 16)
    ap.add_argument("--sample", type=int, default=512, help="rows whose k = 128 lists choose the radii")
    ap.add_argument("--baseline-tree", default=None, help="another built checkout to time embed_knn on, in a child process")
    ap.add_argument("--knn-only", action="store_true", help="(the child's role: embed_knn alone, one JSON line per size)")
    a = ap.parse_args()
    baseline = {}
    if a.baseline_tree and not a.knn_only:  # before this process touches the GPU
        env = dict(os.environ, FEDRANN_BENCH_TREE=os.path.abspath(a.baseline_tree))
        cmd = [sys.executable, os.path.abspath(__file__), "--knn-only", "--dim", str(a.dim), "--k", str(a.k), "--steps",
               str(a.steps), "--reads"] + [str(r) for r in a.reads]
        for line in subprocess.run(cmd, env=env, check=True, capture_output=True, text=True).stdout.splitlines():
            rec = json.loads(line)
            baseline[rec["reads"]] = rec["knn"]
    ctx = _lib.Context(int(os.environ.get("FEDRANN_DEVICE", "0")))
    for R in a.reads:
        cip, cix = _rows(ctx, R, a.dim)
        n = cip.size - 1
        out = {"reads": R, "rows": n, "dim": a.dim, "knn": _knn(ctx, cip, cix, a.k, a.steps)}
        if a.knn_only:
            print(json.dumps(out), flush=True)
            continue
        if R in baseline:
            out["baseline"] = baseline[R]
        blocks = [(lo, min(n, lo + a.block_rows)) for lo in range(0, n, a.block_rows)]
        E = ctx.embed(cip, cix)
        t0 = time.perf_counter()
        with ctx.dense_index_from_csr(cip, cix) as index:
            out["build_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            # the radii: the distance below which the sample's k = 128 lists hold `hits` entries per row
            rows = np.arange(0, n, max(1, n // a.sample))[:a.sample]
            k128 = min(128, n)
            norm = np.sqrt((E.astype(np.float64) ** 2).sum(axis=1))
            Eh = (E / np.where(norm > 0, norm, 1.0)[:, None]).astype(np.float32)
            # (every zero row is a hit of every zero row, at any radius: synth leaves ~2 % of the rows empty)
            out["zero_rows"] = int((norm == 0).sum())
            out["hits_between_zero_rows"] = out["zero_rows"] ** 2
            del E
            parts = []
            for c in range(0, rows.size, 64):  # (on the host, in float32: the radii need no more)
                D = np.clip(1.0 - Eh[rows[c:c + 64]] @ Eh.T, 0.0, 1.0)
                parts.append(np.partition(D, k128 - 1, axis=1)[:, :k128].ravel())
            d = np.sort(np.concatenate(parts))
            del Eh
            d = d[d < 1.0]
            out["block_rows"], out["radii"] = a.block_rows, []
            for h in a.hits:
                radius = float(min(np.float32(d[min(d.size - 1, h * rows.size)]), np.float32(0.999)))

                def radius_search():
                    hits = cand = longest = 0
                    for lo, hi in blocks:
                        ip, _, _ = index.radius_search(radius, lo, hi)
                        info = index.info()
                        hits += info["last_hits"]
                        cand += info["last_candidates"]
                        longest = max(longest, int(np.diff(ip).max()))
                    return hits, cand, longest, info["last_query_blocks"], info["last_segments"]
                ms, ms_all, (scan_ms, tail_ms), (hits, cand, longest, qb, sg) = _timed(ctx, radius_search, a.steps)
                rec = {"aim": h, "radius": round(radius, 6), "hits": hits, "hits_per_query": round(hits / n, 2),
                       "longest_row": longest, "candidates": cand, "cand_per_hit": round(cand / max(hits, 1), 3),
                       "ms": round(ms, 2), "ms_all": ms_all, "device_ms": round(scan_ms + tail_ms, 2),
                       "scan_ms": round(scan_ms, 2), "tail_ms": round(tail_ms, 2),
                       "last_block_grid": [qb, sg], "scan_over_knn_pass": round(scan_ms / max(out["knn"]["knn_pass_ms"], 1e-9), 3),
                       "ms_over_knn_ms": round(ms / out["knn"]["ms"], 3)}
                if R in baseline:
                    rec["ms_over_baseline_ms"] = round(ms / baseline[R]["ms"], 3)
                    rec["scan_over_baseline_pass"] = round(scan_ms / max(baseline[R]["knn_pass_ms"], 1e-9), 3)
                out["radii"].append(rec)
            out["index"] = index.info()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
