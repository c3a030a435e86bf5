"""distributed.sparse_knn_sharded on three ranks that share GPU 0 over a gloo file rendezvous: every rank holds its own
rows only, and the ranks' results, concatenated, are Context.knn_sparse on the whole CSR bit for bit under all three
metrics.  The ranks are child processes (tests/_gpu_sparse_sharded_worker.py); this process opens the GPU after they
have ended."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _gpu_sparse_sharded_worker import METRICS, PRIVATE, sharded_rows, values_of
from fedrann_amd import _lib
from fedrann_amd.distributed import sparse_shard_offsets

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
R, K, BLOCK_ROWS, WORLD = 1500, 20, 700, 3


def _run_ranks(outdir, reads, k):
    rendezvous = os.path.join(str(outdir), "rendezvous")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_gpu_sparse_sharded_worker.py"), str(outdir),
                               rendezvous, str(reads), str(k), str(BLOCK_ROWS), str(rank), str(WORLD)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for rank in range(WORLD)]
    try:
        outs = [p.communicate(timeout=300)[0].decode(errors="replace") for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)


@pytest.fixture(scope="module")
def session(tmp_path_factory):
    """The ranks' results of one group session, then (the ranks gone) the one-GPU answers on the same rows."""
    outdir = tmp_path_factory.mktemp("sharded")
    _run_ranks(outdir, R, K)
    ranks = [np.load(os.path.join(str(outdir), "rank%d.npz" % r)) for r in range(WORLD)]
    indptr, indices, F, weights, blocks = sharded_rows(R, WORLD)
    with _lib.Context(0) as ctx:
        want = {m: ctx.knn_sparse(indptr, indices, values_of(m, weights, indices), F, K, metric=m) for m in METRICS}
    return ranks, want, (indptr, indices, F, blocks)


def test_the_rows_are_what_the_test_is_about():
    indptr, indices, F, weights, blocks = sharded_rows(R, WORLD)
    n = indptr.size - 1
    assert n == 3000 and blocks == [(0, 1024), (1024, 2048), (2048, 3000)]  # ragged query blocks of 700 in each
    lens = np.diff(indptr)
    empty = np.flatnonzero(lens == 0)
    assert {1024, 2999} <= set(empty.tolist()) and all(np.any((empty >= lo) & (empty < hi)) for lo, hi in blocks)
    private = np.flatnonzero((lens == 1) & (indices[np.minimum(indptr[:-1], indices.size - 1)] >= F - PRIVATE))
    assert private.size == PRIVATE and np.any(private >= 2048) and np.any((private >= 1024) & (private < 2048))
    assert np.unique(indices[indptr[private]]).size == PRIVATE and weights.size == F


@pytest.mark.parametrize("metric", METRICS)
def test_three_ranks_give_the_one_gpu_answer(session, metric):
    ranks, want, (indptr, indices, F, blocks) = session
    idx = np.concatenate([z["idx_" + metric] for z in ranks])
    dist = np.concatenate([z["dist_" + metric] for z in ranks])
    assert [(int(z["lo"]), int(z["hi"])) for z in ranks] == blocks
    assert all(z["idx_" + metric].shape == (hi - lo, K) for z, (lo, hi) in zip(ranks, blocks))
    assert idx.dtype == np.int32 and dist.dtype == np.float32
    assert np.array_equal(idx, want[metric][0])
    assert np.array_equal(dist.view(np.uint32), want[metric][1].view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
def test_a_private_row_is_filled_from_rank_zero(session, metric):
    """Self at distance 0, then rows 0 .. K - 2 at distance 1: every candidate but the first comes from another rank."""
    ranks, _, (indptr, indices, F, blocks) = session
    lens = np.diff(indptr)
    private = [r for r in np.flatnonzero(lens == 1) if indices[indptr[r]] >= F - PRIVATE and r >= blocks[1][0]]
    assert private
    for r in private:
        g = [i for i, (lo, hi) in enumerate(blocks) if lo <= r < hi][0]
        row_i, row_d = ranks[g]["idx_" + metric][r - blocks[g][0]], ranks[g]["dist_" + metric][r - blocks[g][0]]
        assert row_i.tolist() == [r] + list(range(K - 1))
        assert row_d[0] < 1e-6 and row_d[1:].tolist() == [1.0] * (K - 1)


def test_k_above_the_smallest_shard_fails_on_every_rank_before_any_index(tmp_path):
    reads, k = 40, 20  # 80 rows: blocks of 32, 32 and 16 rows
    _run_ranks(tmp_path, reads, k)
    blocks = sharded_rows(reads, WORLD)[4]
    counts = [hi - lo for lo, hi in blocks]
    assert counts == [32, 32, 16]
    with pytest.raises(ValueError) as e:
        sparse_shard_offsets(counts, k)
    assert "rank 2 of 3 holds 16 target rows" in str(e.value)
    for rank in range(WORLD):
        with open(os.path.join(str(tmp_path), "rank%d.json" % rank)) as f:
            report = json.load(f)
        assert report["message"] == str(e.value)
        assert report["info_rc"] == -5 and report["metric"] == METRICS[0]  # FDR_E_STATE: no index was built
        assert not os.path.exists(os.path.join(str(tmp_path), "rank%d.npz" % rank))
