"""One rank of tests/test_gpu_sparse_sharded.py: distributed.sparse_knn_sharded on its own rows of the edited synthetic
reads, under all three metrics in one gloo group session (file rendezvous; the ranks share GPU 0).
usage: python _gpu_sparse_sharded_worker.py OUTDIR RENDEZVOUS READS K BLOCK_ROWS RANK WORLD
Writes OUTDIR/rank<r>.npz (lo, hi and idx / dist / seconds per metric), or, where the search is refused,
OUTDIR/rank<r>.json with the message and what fdr_sparse_index_info returned afterwards."""
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedrann_amd.distributed import local_csr, shard_rows  # noqa: E402
from fedrann_amd.precompute import idf_weights  # noqa: E402
from fedrann_amd.synth import synth  # noqa: E402

METRICS = ("cosine", "jaccard", "weighted_jaccard")
PRIVATE = 6  # rows that hold one feature nobody else holds


def sharded_rows(R, world):
    """(indptr, indices, n_features, weights float32 [n_features], blocks) of synth(R, seed=602, doubling=True) with:
    one row emptied in each rank's block (the first row of rank 1 and the last row overall among them), and PRIVATE rows,
    in every rank's block, cut down to one feature of their own (new columns behind the reads' features): such a row's
    list is itself, then the distance-1 fill, rows 0, 1, ... of rank 0's shard."""
    s = synth(R, seed=602, doubling=True)
    indptr, indices, F = s["indptr"], s["indices"], s["n_features"]
    n = indptr.size - 1
    blocks = shard_rows(n, world)[1]
    rows = [indices[indptr[r]:indptr[r + 1]] for r in range(n)]
    empty = sorted({blocks[0][0] + min(17, blocks[0][1] - 1), n - 1} | {lo for lo, hi in blocks[1:] if hi > lo})
    for r in empty:
        rows[r] = indices[:0]
    at = 0
    for g, (lo, hi) in enumerate(blocks):
        for j in range(PRIVATE // world + (g < PRIVATE % world)):
            r = lo + (5 + 97 * j) % max(hi - lo - 2, 1) + 1  # (never a block's first or last row: those may be empty)
            assert r not in empty
            rows[r] = np.array([F + at], np.int32)
            at += 1
    ip = np.zeros(n + 1, np.int64)
    np.cumsum([r.size for r in rows], out=ip[1:])
    weights = np.concatenate([idf_weights(s["counts"], F), np.linspace(0.5, 2.0, at, dtype=np.float32)])
    return ip, np.ascontiguousarray(np.concatenate(rows), dtype=np.int32), F + at, weights, blocks


def values_of(metric, weights, indices):
    """cosine: the IDF values; jaccard: None; weighted_jaccard: the IDF clamped at 0."""
    if metric == "jaccard":
        return None
    w = np.maximum(weights, np.float32(0)) if metric == "weighted_jaccard" else weights
    return np.ascontiguousarray(w[indices])


def main():
    import torch.distributed as dist
    from fedrann_amd import _lib
    from fedrann_amd.distributed import sparse_knn_sharded
    outdir, rendezvous = sys.argv[1:3]
    R, k, block_rows, rank, world = (int(a) for a in sys.argv[3:8])
    indptr, indices, F, weights, blocks = sharded_rows(R, world)
    lo, hi = blocks[rank]
    ip, ix = local_csr(indptr, indices, lo, hi)  # from here on the rank knows its own rows only
    del indptr, indices
    dist.init_process_group("gloo", init_method="file://" + rendezvous, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    out = {}
    try:
        with _lib.Context(0) as ctx:
            for metric in METRICS:
                t0 = time.perf_counter()
                try:
                    glo, ghi, idx, dst = sparse_knn_sharded(ctx, ip, ix, values_of(metric, weights, ix), F, k,
                                                            metric=metric, block_rows=block_rows)
                except ValueError as e:
                    rc = ctx._L.fdr_sparse_index_info(ctx._h, None, None, None, None, None)
                    with open(os.path.join(outdir, "rank%d.json" % rank), "w") as f:
                        json.dump({"message": str(e), "info_rc": rc, "metric": metric}, f)
                    return
                assert (glo, ghi) == (lo, hi)
                out["idx_" + metric], out["dist_" + metric] = idx, dst
                out["seconds_" + metric] = time.perf_counter() - t0  # (for the record: docs/experiments.md)
                rc = ctx._L.fdr_sparse_index_info(ctx._h, None, None, None, None, None)
                assert rc == -5, rc  # FDR_E_STATE: the index is freed before the function returns
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), lo=lo, hi=hi, **out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
