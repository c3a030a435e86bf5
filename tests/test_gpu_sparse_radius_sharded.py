"""distributed.sparse_radius_sharded on three ranks that share GPU 0 over a gloo file rendezvous: every rank holds its
own rows only, and the ranks' ragged results, concatenated, are SparseIndex.radius_search on the whole CSR bit for bit
under all three metrics.  The ranks are child processes (tests/_gpu_sparse_radius_sharded_worker.py); this process
opens the GPU after they have ended."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _radius_model as rmodel
from _gpu_sparse_radius_sharded_worker import tag
from _gpu_sparse_sharded_worker import METRICS, PRIVATE, sharded_rows, values_of
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
R, BLOCK_ROWS, WORLD = 1500, 700, 3
RADII = (0.0, 0.5, 0.9)
BAD_RADIUS = 1.5


def _run_ranks(outdir, max_hits, metrics, radii):
    rendezvous = os.path.join(str(outdir), "rendezvous")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_gpu_sparse_radius_sharded_worker.py"), str(outdir),
                               rendezvous, str(R), str(BLOCK_ROWS), str(max_hits), str(rank), str(WORLD),
                               ",".join(metrics)] + ["%g" % r for r in radii],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for rank in range(WORLD)]
    try:
        outs = [p.communicate(timeout=300)[0].decode(errors="replace") for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    return [np.load(os.path.join(str(outdir), "rank%d.npz" % r)) for r in range(WORLD)]


def _capped_run_cap(indptr, indices, F, blocks):
    """A cap on the hits of one device call for the Jaccard search at 0.9, from the CPU model: the fullest row's hits
    over ALL targets (so every rank's row and every merged row fits), which is below what the fullest (query block,
    rank) pair holds, so some rank has to cut a block by its counts."""
    D = rmodel.distances("jaccard", (indptr, indices, None), (indptr, indices, None), F) <= np.float32(0.9)
    cap = int(D.sum(axis=1).max())
    per_call = [int(D[a:min(b, a + BLOCK_ROWS), lo:hi].sum()) for lo, hi in blocks for s0, b in blocks
                for a in range(s0, b, BLOCK_ROWS)]
    assert cap < max(per_call)
    return cap


@pytest.fixture(scope="module")
def session(tmp_path_factory):
    """The ranks' results of two group sessions (every metric and radius; Jaccard under a cap, after a refused radius),
    then (the ranks gone) the one-GPU answers on the same rows."""
    indptr, indices, F, weights, blocks = sharded_rows(R, WORLD)
    ranks = _run_ranks(tmp_path_factory.mktemp("sharded"), 1 << 26, METRICS, RADII)
    capped_dir = tmp_path_factory.mktemp("capped")
    cap = _capped_run_cap(indptr, indices, F, blocks)
    capped = _run_ranks(capped_dir, cap, ["jaccard"], (BAD_RADIUS, 0.9))
    reports = [json.load(open(os.path.join(str(capped_dir), "rank%d.json" % r))) for r in range(WORLD)]
    want = {}
    with _lib.Context(0) as ctx:
        for m in METRICS:
            with ctx.sparse_index(indptr, indices, values_of(m, weights, indices), F, metric=m) as index:
                for r in RADII:
                    want[tag(m, r)] = index.radius_search(r)
    return ranks, capped, reports, want, (indptr, indices, F, blocks)


def _joined(ranks, t):
    ip = np.zeros(1, np.int64)
    for z in ranks:
        ip = np.concatenate([ip, ip[-1] + z["indptr_" + t][1:]])
    return ip, np.concatenate([z["idx_" + t] for z in ranks]), np.concatenate([z["dist_" + t] for z in ranks])


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("metric", METRICS)
def test_three_ranks_give_the_one_gpu_answer(session, metric, r):
    ranks, _, _, want, (indptr, indices, F, blocks) = session
    t = tag(metric, r)
    assert [(int(z["lo"]), int(z["hi"])) for z in ranks] == blocks
    assert all(z["indptr_" + t].shape == (hi - lo + 1,) and z["indptr_" + t][0] == 0 for z, (lo, hi) in zip(ranks, blocks))
    rmodel.same(_joined(ranks, t), want[t])
    if metric == "jaccard" and r in (0.5, 0.9):  # (the totals of the CPU model: tests/test_radius_merge_host.py)
        assert int(want[t][0][-1]) == {0.5: 19_780, 0.9: 142_970}[r]
    print("sparse_radius_sharded %s: %.3f s on the slowest rank, %d hits"
          % (t, max(float(z["seconds_" + t]) for z in ranks), int(want[t][0][-1])))


def test_a_cap_below_the_fullest_block_gives_the_same_rows(session):
    ranks, capped, _, want, _ = session
    rmodel.same(_joined(capped, tag("jaccard", 0.9)), want[tag("jaccard", 0.9)])


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("metric", METRICS)
def test_empty_and_private_rows(session, metric, r):
    """An empty row returns the four empty rows, spread over all three ranks, at distance 0; a row that holds one
    feature nobody else holds returns itself only."""
    ranks, _, _, _, (indptr, indices, F, blocks) = session
    lens = np.diff(indptr)
    empty = np.flatnonzero(lens == 0)
    assert empty.size == 4 and all(np.any((empty >= lo) & (empty < hi)) for lo, hi in blocks)
    private = [q for q in np.flatnonzero(lens == 1) if indices[indptr[q]] >= F - PRIVATE]
    assert len(private) == PRIVATE
    ip, ix, ds = _joined(ranks, tag(metric, r))
    for q in empty:
        assert ix[ip[q]:ip[q + 1]].tolist() == empty.tolist() and np.all(ds[ip[q]:ip[q + 1]] == 0)
    for q in private:
        row = ix[ip[q]:ip[q + 1]].tolist()
        # (its own distance is 0 up to the rounding of a cosine, below 1e-6 as in the k-NN test: at r = 0 the row holds
        # itself where that rounding gives exactly 0, and nothing else either way)
        assert row == [q] or (r == 0.0 and metric == "cosine" and row == [])
        assert np.all(ds[ip[q]:ip[q + 1]] < 1e-6)


def test_a_bad_radius_fails_on_every_rank_before_any_index(session):
    _, _, reports, _, _ = session
    with pytest.raises(ValueError) as e:
        _lib.check_sparse_radius(BAD_RADIUS, 1 << 26)
    for report in reports:
        assert report["message"] == str(e.value) and report["radius"] == BAD_RADIUS and report["metric"] == "jaccard"
        assert report["info_rc"] == -5  # FDR_E_STATE: the first search of the session, and no index was built
