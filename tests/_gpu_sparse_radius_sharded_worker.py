"""One rank of tests/test_gpu_sparse_radius_sharded.py: distributed.sparse_radius_sharded on its own rows of the edited
synthetic reads (the rows of _gpu_sparse_sharded_worker), under the metrics and the radii given, in one gloo group
session (file rendezvous; the ranks share GPU 0).
usage: python _gpu_sparse_radius_sharded_worker.py OUTDIR RENDEZVOUS READS BLOCK_ROWS MAX_HITS RANK WORLD METRICS RADIUS...
(METRICS: names joined by commas.)  Writes OUTDIR/rank<r>.npz (lo, hi and indptr / idx / dist / seconds per metric and
radius) and, where a search is refused, OUTDIR/rank<r>.json with the message and what fdr_sparse_index_info returned
right afterwards; the rank goes on with the next search."""
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _gpu_sparse_sharded_worker import sharded_rows, values_of  # noqa: E402
from fedrann_amd.distributed import local_csr  # noqa: E402


def tag(metric, radius):
    return "%s_%g" % (metric, radius)


def main():
    import torch.distributed as dist
    from fedrann_amd import _lib
    from fedrann_amd.distributed import sparse_radius_sharded
    outdir, rendezvous = sys.argv[1:3]
    R, block_rows, max_hits, rank, world = (int(a) for a in sys.argv[3:8])
    metrics = sys.argv[8].split(",")
    radii = [float(a) for a in sys.argv[9:]]
    indptr, indices, F, weights, blocks = sharded_rows(R, world)
    lo, hi = blocks[rank]
    ip, ix = local_csr(indptr, indices, lo, hi)  # from here on the rank knows its own rows only
    del indptr, indices
    dist.init_process_group("gloo", init_method="file://" + rendezvous, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    out = {}
    try:
        with _lib.Context(0) as ctx:
            for metric in metrics:
                for radius in radii:
                    t0 = time.perf_counter()
                    try:
                        glo, ghi, rip, idx, dst = sparse_radius_sharded(
                            ctx, ip, ix, values_of(metric, weights, ix), F, radius, metric=metric,
                            block_rows=block_rows, max_hits=max_hits)
                    except ValueError as e:
                        rc = ctx._L.fdr_sparse_index_info(ctx._h, None, None, None, None, None)
                        with open(os.path.join(outdir, "rank%d.json" % rank), "w") as f:
                            json.dump({"message": str(e), "info_rc": rc, "metric": metric, "radius": radius}, f)
                        continue
                    assert (glo, ghi) == (lo, hi)
                    t = tag(metric, radius)
                    out["indptr_" + t], out["idx_" + t], out["dist_" + t] = rip, idx, dst
                    out["seconds_" + t] = time.perf_counter() - t0  # (for the record: docs/experiments.md)
                    rc = ctx._L.fdr_sparse_index_info(ctx._h, None, None, None, None, None)
                    assert rc == -5, rc  # FDR_E_STATE: the index is freed before the function returns
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), lo=lo, hi=hi, **out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
