"""`--rescore METRIC --rescore-candidates K'` in the default, projected mode: overlaps.tsv of the command line equals,
byte for byte, the file write_overlaps makes of the lists of Context.embed_knn at K' re-scored by the numpy MODEL of the
sparse search under METRIC (tests/_sparse_query_model.py), on a tiny feature matrix; and a run without the flag writes
the file it wrote before."""
import numpy as np
import pytest

import _sparse_query_model as qmodel
from fedrann_amd import __main__ as cli
from fedrann_amd import feature_extraction as fx
from fedrann_amd.precompute import build_precompute_matrix
from fedrann_amd.synth import synth

pytestmark = pytest.mark.gpu

K, KP, D_EMBED = 7, 19, 128


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rescore_cli")
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
    argv = ["-n", str(D_EMBED), "--nndescent-n-neighbors", str(K), "--feature-matrix", str(npz), "--kmer-counts",
            str(counts), "--read-names", str(names)]
    return s, indptr, indices, n_features, argv


@pytest.fixture(scope="module")
def projected(ctx, inputs):
    """k -> the lists of the projected search, as the command line runs it"""
    s, indptr, indices, n_features, _ = inputs
    P = fx._projection_csr(build_precompute_matrix(s["counts"], D_EMBED, n_features=n_features))
    ctx.projection_load(P.indptr, P.indices, P.data, n_features, D_EMBED)
    cip, cix = ctx.csr_compact(indptr, indices)
    return {k: ctx.embed_knn(cip, cix, k) for k in (K, KP)}


def _rescored(D, cand, k):
    idx = np.empty((cand.shape[0], k), np.int32)
    dist = np.empty((cand.shape[0], k), np.float32)
    for q in range(cand.shape[0]):
        d = D[q, cand[q]]
        order = np.lexsort((cand[q], d.view(np.uint32)))[:k]  # (last key first: distance bits, then index)
        idx[q], dist[q] = cand[q][order], d[order]
    return idx, dist


@pytest.mark.parametrize("metric", ["jaccard", "weighted_jaccard"])
def test_cli_rescore_equals_the_model_rescored_lists(tmp_path, inputs, projected, metric):
    s, indptr, indices, n_features, argv = inputs
    if metric == "jaccard":
        D = qmodel.jaccard_distances((indptr, indices, None), (indptr, indices, None), n_features)
    else:
        values = cli.sparse_weights(s["counts"], n_features, metric)[indices]
        D = qmodel.weighted_jaccard_distances((indptr, indices, values), (indptr, indices, values))
    cand = projected[KP][0]
    idx, dist = _rescored(D, cand, K)
    assert np.any(idx != projected[K][0])  # (the exact metric ranks some read's neighbours differently)
    out_dir = tmp_path / "out"
    cli.main(["-o", str(out_dir), "--rescore", metric, "--rescore-candidates", str(KP)] + argv)
    want = tmp_path / "want.tsv"
    lines = cli.write_overlaps(str(want), idx, dist, s["names"], s["strands"])
    assert lines >= 600 * (K - 1)
    assert open(out_dir / "overlaps.tsv", "rb").read() == want.read_bytes()
    assert "K' = %d" % KP in open(out_dir / "fedrann.log").read()


def test_cli_without_the_flag_writes_the_projected_lists(tmp_path, inputs, projected):
    s, _, _, _, argv = inputs
    out_dir = tmp_path / "out"
    cli.main(["-o", str(out_dir)] + argv)
    want = tmp_path / "want.tsv"
    cli.write_overlaps(str(want), *projected[K], s["names"], s["strands"])
    assert open(out_dir / "overlaps.tsv", "rb").read() == want.read_bytes()


def test_cli_refuses_more_candidates_than_reads(tmp_path, inputs):
    """K' <= the number of reads can only be checked once they are loaded: 110 reads, K' = 128"""
    s, indptr, indices, n_features, argv = inputs
    npz = tmp_path / "short.npz"
    fx.save_feature_matrix_npz(str(npz), indptr[:111], indices[:indptr[110]], n_features)
    counts = argv[argv.index("--kmer-counts") + 1]
    with pytest.raises(SystemExit, match="110 reads"):
        cli.main(["-o", str(tmp_path / "out"), "-n", str(D_EMBED), "--nndescent-n-neighbors", "100", "--rescore", "jaccard",
                  "--rescore-candidates", "128", "--feature-matrix", str(npz), "--kmer-counts", counts])
    assert not (tmp_path / "out" / "overlaps.tsv").exists()
