"""Time the merge of the ranks' ragged rows of a target-sharded sparse radius search: Context.radius_merge
(fdr_radius_merge, host to host: the host's indptr pass, upload of the parts, kernel, results back) beside
distributed.merge_sparse_radius (numpy) on the same rows, and beside the bare upload of the same bytes.

    python devtools/bench_radius_merge.py [--queries 125000] [--parts 8] [--hits 5] [--reps 9] [--long-row 0]

The default shape is one rank's share of 1 M rows on 8 ranks, the shape fdr_topk_merge was recorded at, at about --hits
hits per query and part (row lengths Poisson around it, zeros among them).  Rows as in tests/test_gpu_radius_merge.py:
distances from {0, 0.25, 0.5}, distinct indices dealt to the parts, rows sorted by key.  --long-row N makes query 0 a row
of N entries in every part: what one long row costs under the wave-per-query mapping.  Two warm-up calls, then --reps
timed ones each: Context.radius_merge on the parts as a rank holds them (it concatenates them first), the raw call on
arrays concatenated beforehand, pageable and pinned (Context.host_register); prints median (min - max) and checks that
the two merges agree bit for bit.  The kernel alone is not timed here: take one
`rocprofv3 --kernel-trace --stats` run of this script and read radius_merge_kernel's row."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.distributed import merge_sparse_radius  # noqa: E402


def ragged(nq, n_parts, hits, long_row=0, seed=1):
    """n_parts parts (indptr, idx, dist), built without a Python loop over the queries: every entry of a query gets a
    distinct index (a random permutation inside the query), then each part's entries are sorted by (query, key)."""
    rng = np.random.default_rng(seed)
    lens = rng.poisson(hits, size=(n_parts, nq)).astype(np.int64)
    if long_row:
        lens[:, 0] = long_row
    per_query = lens.sum(axis=0)
    q_start = np.zeros(nq + 1, np.int64)
    np.cumsum(per_query, out=q_start[1:])
    total = int(q_start[-1])
    query = np.repeat(np.arange(nq, dtype=np.int64), per_query)
    # a random order of each query's entries: sort (query, random) and take the rank inside the query as the index
    order = np.lexsort((rng.random(total), query))
    index = np.empty(total, np.int32)
    index[order] = (np.arange(total, dtype=np.int64) - q_start[query]).astype(np.int32) * 3 + 1
    dist = rng.choice(np.array([0.0, 0.25, 0.5], np.float32), size=total)
    # deal them to the parts: inside a query, the first lens[0, q] entries to part 0, ...
    part_end = np.cumsum(lens, axis=0)  # [n_parts, nq]
    within = np.arange(total, dtype=np.int64) - q_start[query]
    part = np.zeros(total, np.int8)
    for p in range(n_parts - 1):
        part += within >= part_end[p][query]
    parts = []
    for p in range(n_parts):
        sel = np.flatnonzero(part == p)
        key = (dist[sel].view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[sel].astype(np.uint32)
        o = sel[np.lexsort((key, query[sel]))]
        ip = np.zeros(nq + 1, np.int64)
        np.cumsum(lens[p], out=ip[1:])
        parts.append((ip, np.ascontiguousarray(index[o]), np.ascontiguousarray(dist[o])))
    return parts


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
    ap.add_argument("--hits", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--long-row", type=int, default=0)
    ap.add_argument("--no-numpy", action="store_true", help="skip the numpy merge (and the comparison)")
    a = ap.parse_args()
    parts = ragged(a.queries, a.parts, a.hits, a.long_row)
    total = sum(int(p[0][-1]) for p in parts)
    mb = 8 * total / 1e6
    import torch
    flat_i = np.concatenate([p[1] for p in parts])
    flat_d = np.concatenate([p[2] for p in parts])
    dev = torch.empty(2 * total, dtype=torch.int32, device="cuda")

    def upload():
        dev[:total].copy_(torch.from_numpy(flat_i))
        dev[total:].view(torch.float32).copy_(torch.from_numpy(flat_d))
        torch.cuda.synchronize()
    _, u_med, u_min, u_max = timed(upload, a.reps)
    with _lib.Context(0) as ctx:
        got, g_med, g_min, g_max = timed(lambda: ctx.radius_merge(parts, max_entries=2 ** 31 - 1), a.reps)
        ips = np.stack([p[0] for p in parts])
        out = np.empty(a.queries + 1, np.int64), np.empty(total, np.int32), np.empty(total, np.float32)

        def raw():
            ctx._check(ctx._L.fdr_radius_merge(ctx._h, a.queries, a.parts, _lib._ptr(ips), _lib._ptr(flat_i),
                                               _lib._ptr(flat_d), _lib._ptr(out[0]), _lib._ptr(out[1]), _lib._ptr(out[2])),
                       "fdr_radius_merge")
        _, r_med, r_min, r_max = timed(raw, a.reps)
        ctx.host_register(flat_i, flat_d, out[1], out[2])
        try:
            _, p_med, p_min, p_max = timed(raw, a.reps)
        finally:
            ctx.host_unregister(flat_i, flat_d, out[1], out[2])
        assert all(np.array_equal(g.view(np.uint32), o.view(np.uint32)) for g, o in zip(got[1:], out[1:]))
    print("%d queries x %d parts, about %g hits per query and part%s: %d entries (%.1f MB of parts), %d reps"
          % (a.queries, a.parts, a.hits, ", query 0 with %d per part" % a.long_row if a.long_row else "", total, mb,
             a.reps))
    print("bare upload of the entries (torch, pageable):   %.2f ms (%.2f - %.2f)" % (u_med, u_min, u_max))
    print("Context.radius_merge (concatenates the parts):  %.2f ms (%.2f - %.2f)" % (g_med, g_min, g_max))
    print("fdr_radius_merge, concatenated, pageable:       %.2f ms (%.2f - %.2f)" % (r_med, r_min, r_max))
    print("fdr_radius_merge, concatenated, pinned:         %.2f ms (%.2f - %.2f)" % (p_med, p_min, p_max))
    if a.no_numpy:
        return 0
    want, n_med, n_min, n_max = timed(lambda: merge_sparse_radius(parts), min(a.reps, 3), warmup=0)
    same = all(np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                              w.view(np.uint32) if w.dtype == np.float32 else w) for g, w in zip(got, want))
    print("merge_sparse_radius (numpy):                    %.2f ms (%.2f - %.2f)" % (n_med, n_min, n_max))
    print("bit for bit the same: %s" % same)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
