"""Time Context.graph_symmetrize (fdr_graph_symmetrize + fdr_graph_symmetrize_fetch, host to host: the host's indptr
pass, the upload, four kernels and two segmented sorts, the result back) beside graph.symmetrize_rows (numpy) on the same
graph, in the same process, for the three modes.

    python devtools/bench_graph_symmetrize.py [--shape knn100k knn1m ragged100k] [--mode union mutual transpose]
                                              [--reps 7] [--numpy-reps 1]

Shapes: k-NN-like graphs of 100 000 x 20 and 1 000 000 x 20 with half of every row's pairs reciprocated, and a ragged
one of 100 000 rows with about 100 entries each (Binomial(200, 1/2)), again about half reciprocated.  Every row lists
the rows at a fixed set of offsets from it, under a random relabelling of the rows, so a row's targets are spread over
the whole graph as a search's are; the distances are random and differ between the two directions.  One warm-up call,
then --reps timed ones: median (min - max).  The result is checked against the model bit for bit.  The kernels alone
are not timed here (the library has no timing slot for them): take one `rocprofv3 --kernel-trace --stats` run of this
script with one --shape, one --mode and --numpy-reps 0, and read the gs_*_kernel, radius_split_kernel and rocprim rows."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.graph import symmetrize_rows  # noqa: E402

MODES = ("union", "mutual", "transpose")


def _offsets(rng, n, pairs, one_way):
    """`pairs` offsets taken with their negatives (reciprocated), `one_way` more whose negatives are not taken"""
    o = rng.choice(np.arange(1, (n - 1) // 2), size=pairs + one_way, replace=False).astype(np.int64)
    return np.concatenate([o[:pairs], -o[:pairs], o[pairs:]])


def knn_like(n, k, seed=1):
    """(idx int32 [n, k], dist float32 [n, k]): k / 2 of each row's entries have their reverse in the graph"""
    rng = np.random.default_rng(seed)
    off = _offsets(rng, n, k // 4, k - 2 * (k // 4))
    relabel = rng.permutation(n).astype(np.int64)
    idx = np.empty((n, k), np.int32)
    idx[relabel] = relabel[(np.arange(n, dtype=np.int64)[:, None] + off[None, :]) % n]
    return idx, rng.random((n, k), dtype=np.float32)


def ragged(n, mean, seed=2):
    """(indptr, idx, dist): each of 2 * mean offsets (mean reciprocal pairs) kept with probability 1/2 per row"""
    rng = np.random.default_rng(seed)
    off = _offsets(rng, n, mean, 0)
    relabel = rng.permutation(n).astype(np.int64)
    keep = rng.random((n, off.size)) < 0.5
    full = np.empty((n, off.size), np.int32)
    full[relabel] = relabel[(np.arange(n, dtype=np.int64)[:, None] + off[None, :]) % n]
    kept = np.empty_like(keep)
    kept[relabel] = keep
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(kept.sum(axis=1), out=indptr[1:])
    idx = np.ascontiguousarray(full[kept])
    return indptr, idx, rng.random(idx.size, dtype=np.float32)


SHAPES = {"knn100k": lambda: knn_like(100_000, 20), "knn1m": lambda: knn_like(1_000_000, 20),
          "ragged100k": lambda: ragged(100_000, 100)}


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        out = fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), min(t), max(t)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", nargs="+", choices=sorted(SHAPES), default=["knn100k", "knn1m", "ragged100k"])
    ap.add_argument("--mode", nargs="+", choices=MODES, default=list(MODES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--numpy-reps", type=int, default=1, help="0: skip the numpy model (and the comparison)")
    a = ap.parse_args()
    ok = True
    with _lib.Context(0) as ctx:
        for shape in a.shape:
            graph = SHAPES[shape]()
            _, n, ip, ix, ds = _lib.check_graph_symmetrize(graph)
            print("%s: %d rows, %d entries (%.1f MB up), %d reps" % (shape, n, ix.size, 8 * ix.size / 1e6, a.reps), flush=True)
            for mode in a.mode:
                got, med, lo, hi = timed(lambda: ctx.graph_symmetrize(graph, mode, max_entries=2 ** 31 - 1), a.reps)
                line = "  %-9s %9d entries out   GPU, host to host: %8.2f ms (%.2f - %.2f)" % (mode, got[1].size, med, lo, hi)
                if a.numpy_reps:
                    want, nmed, nlo, nhi = timed(lambda: symmetrize_rows(ip, ix, ds, mode), a.numpy_reps, warmup=0)
                    same = all(np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                              w.view(np.uint32) if w.dtype == np.float32 else w) for g, w in zip(got, want))
                    ok = ok and same
                    line += "   numpy: %9.1f ms (%.1f - %.1f)   bit for bit the same: %s" % (nmed, nlo, nhi, same)
                print(line, flush=True)
            ctx.graph_free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
