"""Time the merge of the ranks' candidate lists of a target-sharded sparse search: Context.topk_merge (fdr_topk_merge,
host to host: upload of the parts, kernel, results back) beside distributed.merge_sparse_topk (numpy) on the same lists.

    python devtools/bench_topk_merge.py [--queries 125000] [--parts 8] [--kp 20] [-k 20] [--reps 9]

The default shape is one rank's share of 1 M rows on 8 ranks at k = 20.  Lists as in tests/test_gpu_topk_merge.py:
distances from {0, 0.25, 1}, distinct indices dealt to the parts, rows sorted by key.  Two warm-up calls, then --reps
timed ones each, the device merge from pageable and from pinned (Context.host_register) host arrays; prints median
(min - max) and checks that the two merges agree bit for bit."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.distributed import merge_sparse_topk  # noqa: E402


def lists(nq, n_parts, kp, seed=1):
    rng = np.random.default_rng(seed)
    slots = n_parts * kp
    pool = np.tile(np.arange(slots + 37, dtype=np.int32), (nq, 1))
    idx = np.ascontiguousarray(rng.permuted(pool, axis=1)[:, :slots].reshape(nq, n_parts, kp).transpose(1, 0, 2))
    dist = rng.choice(np.array([0.0, 0.25, 1.0], np.float32), size=(n_parts, nq, kp))
    key = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint32)
    order = np.argsort(key, axis=-1, kind="stable")
    return (np.ascontiguousarray(np.take_along_axis(idx, order, axis=-1)),
            np.ascontiguousarray(np.take_along_axis(dist, order, axis=-1)))


def timed(fn, reps, warmup=2):
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
    ap.add_argument("--queries", type=int, default=125_000)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--kp", type=int, default=20)
    ap.add_argument("-k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    idx_parts, dist_parts = lists(a.queries, a.parts, a.kp)
    parts = [(idx_parts[p], dist_parts[p]) for p in range(a.parts)]
    mb = 2 * idx_parts.nbytes / 1e6
    with _lib.Context(0) as ctx:
        out = np.empty((a.queries, a.k), np.int32), np.empty((a.queries, a.k), np.float32)
        got, g_med, g_min, g_max = timed(lambda: ctx.topk_merge(idx_parts, dist_parts, a.k, out=out), a.reps)
        ctx.host_register(idx_parts, dist_parts, out[0], out[1])
        try:
            _, p_med, p_min, p_max = timed(lambda: ctx.topk_merge(idx_parts, dist_parts, a.k, out=out), a.reps)
        finally:
            ctx.host_unregister(idx_parts, dist_parts, out[0], out[1])
    want, n_med, n_min, n_max = timed(lambda: merge_sparse_topk(parts, a.k), a.reps)
    same = np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    print("%d queries x %d parts x %d candidates, k = %d (%.1f MB of parts), %d reps" % (a.queries, a.parts, a.kp, a.k, mb,
                                                                                          a.reps))
    print("Context.topk_merge, pageable host arrays: %.2f ms (%.2f - %.2f)" % (g_med, g_min, g_max))
    print("Context.topk_merge, pinned host arrays:   %.2f ms (%.2f - %.2f)" % (p_med, p_min, p_max))
    print("merge_sparse_topk (numpy):                %.2f ms (%.2f - %.2f)" % (n_med, n_min, n_max))
    print("bit for bit the same: %s" % same)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
