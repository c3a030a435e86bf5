"""`--radius R --radius-rescore METRIC [--radius-rescore-bound R2]` in the default, projected mode: overlaps.tsv of the
command line equals, byte for byte, the file overlaps_write_csr makes of the rows of DenseIndex.radius_search(R)
re-scored by the numpy MODEL of the sparse search under METRIC (tests/_sparse_query_model.py, tests/_radius_model.py)
and cut at R2, on a tiny feature matrix."""
import numpy as np
import pytest

import _radius_model as rmodel
import _rescore_rows as rr
import _sparse_query_model as qmodel
from fedrann_amd import __main__ as cli
from fedrann_amd import _lib
from fedrann_amd import feature_extraction as fx
from fedrann_amd.precompute import build_precompute_matrix
from fedrann_amd.synth import synth

pytestmark = pytest.mark.gpu

D_EMBED, R = 128, 0.6


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("radius_rescore_cli")
    s = synth(600, seed=9, m=60, doubling=True)
    npz = tmp / "feature_matrix.npz"
    fx.save_feature_matrix_npz(str(npz), s["indptr"], s["indices"], s["n_features"])
    counts = tmp / "counts.npy"
    np.save(counts, s["counts"])
    names = tmp / "names.txt"
    with open(names, "w") as f:
        for n, st in zip(s["names"], s["strands"]):
            f.write("%s\t%d\n" % (n, st))
    indptr, indices, n_features = fx.load_feature_matrix_npz(str(npz))
    argv = ["-n", str(D_EMBED), "--feature-matrix", str(npz), "--kmer-counts", str(counts), "--read-names", str(names)]
    return s, indptr, indices, n_features, argv


@pytest.fixture(scope="module")
def projected(ctx, inputs):
    """the rows of the projected radius search, as the command line runs it"""
    s, indptr, indices, n_features, _ = inputs
    P = fx._projection_csr(build_precompute_matrix(s["counts"], D_EMBED, n_features=n_features))
    ctx.projection_load(P.indptr, P.indices, P.data, n_features, D_EMBED)
    cip, cix = ctx.csr_compact(indptr, indices)
    with ctx.dense_index_from_csr(cip, cix) as index:
        return index.radius_search(R)


def _matrix(metric, oracle, s, indptr, indices, n_features):
    if metric == "jaccard":
        return qmodel.jaccard_distances((indptr, indices, None), (indptr, indices, None), n_features)
    values = cli.sparse_weights(s["counts"], n_features, metric)[indices]
    return rr.matrix(metric, oracle, (indptr, indices, values), n_features)


@pytest.mark.parametrize("metric, bound", [("jaccard", 0.9), ("cosine", None)])
def test_cli_equals_the_model_rescored_rows(tmp_path, oracle, inputs, projected, metric, bound):
    s, indptr, indices, n_features, argv = inputs
    cand_ip, cand_ix, _ = projected
    D = _matrix(metric, oracle, s, indptr, indices, n_features)
    ip, idx, dist = rr.want(D, 0, cand_ip, cand_ix, 1.0 if bound is None else bound)
    if bound is None:  # every projected hit, with the exact distances in the exact order
        assert np.array_equal(ip, cand_ip) and not np.array_equal(idx, cand_ix)
    else:
        assert 0 < ip[-1] < cand_ip[-1]
    assert cand_ip[-1] > 600  # (more than the reads themselves)
    out_dir = tmp_path / "out"
    cli.main(["-o", str(out_dir), "--radius", str(R), "--radius-rescore", metric] + argv
             + ([] if bound is None else ["--radius-rescore-bound", str(bound)]))
    want = tmp_path / "want.tsv"
    name_off, names = _lib.pack_names(s["names"])
    lines = _lib.overlaps_write_csr(str(want), ip, idx, dist, name_off, names, np.asarray(s["strands"], np.uint8))
    assert lines > 0
    assert open(out_dir / "overlaps.tsv", "rb").read() == want.read_bytes()
    assert "re-scored on the feature rows (metric = %s" % metric in open(out_dir / "fedrann.log").read()


def test_cli_in_blocks_writes_the_same_file(tmp_path, monkeypatch, inputs):
    """row blocks and pieces under the cap change no byte"""
    _, _, _, _, argv = inputs
    args = ["--radius", str(R), "--radius-rescore", "weighted_jaccard", "--radius-rescore-bound", "0.95"] + argv
    cli.main(["-o", str(tmp_path / "whole")] + args)
    monkeypatch.setattr(cli, "RADIUS_BLOCK_ROWS", 250)
    monkeypatch.setattr(cli, "RADIUS_MAX_HITS", 4000)
    cli.main(["-o", str(tmp_path / "blocks")] + args)
    whole = open(tmp_path / "whole" / "overlaps.tsv", "rb").read()
    assert whole.count(b"\n") > 600 and whole == open(tmp_path / "blocks" / "overlaps.tsv", "rb").read()
