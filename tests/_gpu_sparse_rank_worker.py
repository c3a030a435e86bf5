"""One rank of tests/test_gpu_sparse_index.py::test_three_ranks_tile_the_whole_call: sparse_knn_rank on synthetic reads
with IDF values.  No process group: the ranks share GPU 0 and nothing else.
usage: python _gpu_sparse_rank_worker.py OUTDIR READS K BLOCK_ROWS RANK WORLD"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.distributed import sparse_knn_rank  # noqa: E402
from fedrann_amd.precompute import idf_weights  # noqa: E402
from fedrann_amd.synth import synth  # noqa: E402

outdir, R, k, block_rows, rank, world = sys.argv[1], *(int(a) for a in sys.argv[2:7])
s = synth(R, seed=602, doubling=True)
values = idf_weights(s["counts"], s["n_features"])[s["indices"]]
with _lib.Context(0) as ctx:
    lo, hi, idx, dist = sparse_knn_rank(ctx, s["indptr"], s["indices"], values, s["n_features"], k, rank, world,
                                        block_rows=block_rows)
    trace = ctx.last_knn_trace()
np.savez(os.path.join(outdir, "rank%d.npz" % rank), lo=lo, hi=hi, idx=idx, dist=dist, queries=trace["queries"],
         targets=trace["targets"])
