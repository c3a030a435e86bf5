"""`--refine METRIC [--refine-fan F] [--refine-rounds T] [--refine-reverse]` in the default, projected mode:
overlaps.tsv of the command line equals, byte for byte, the file fdr_overlaps_write_csr makes of T RescoreRows.refine
calls on the lists of the projected search, on the tiny feature matrix of tests/test_gpu_cli_rescore.py; and every
refused combination of flags exits with its message before any work."""
import numpy as np
import pytest

from fedrann_amd import __main__ as cli
from fedrann_amd import _lib
from fedrann_amd import feature_extraction as fx
from fedrann_amd.precompute import build_precompute_matrix
from fedrann_amd.synth import synth

pytestmark = pytest.mark.gpu

K, KP, D_EMBED = 7, 19, 128


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("refine_cli")
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


def _written(path, graph, s):
    name_off, names = _lib.pack_names(s["names"])
    return _lib.overlaps_write_csr(str(path), *graph, name_off, names, np.asarray(s["strands"], np.uint8))


def test_two_rounds_write_what_two_refine_calls_on_the_projected_lists_give(ctx, tmp_path, inputs, projected):
    s, indptr, indices, n_features, argv = inputs
    out_dir = tmp_path / "out"
    cli.main(["-o", str(out_dir), "--refine", "jaccard", "--refine-rounds", "2"] + argv)
    with ctx.rescore_rows(indptr, indices, None, n_features, metric="jaccard") as held:
        once = held.refine(projected[K], K)
        twice = held.refine(once, K)
    assert np.all(np.diff(twice[0]) <= K) and not np.array_equal(once[1], projected[K][0].reshape(-1))
    want = tmp_path / "want.tsv"
    assert _written(want, twice, s) >= 600 * (K - 1)
    assert open(out_dir / "overlaps.tsv", "rb").read() == want.read_bytes()
    log = open(out_dir / "fedrann.log").read()
    assert "round 1 of 2" in log and "round 2 of 2" in log


def test_after_a_rescore_with_a_fan_the_reverse_neighbours_and_a_symmetrise(ctx, tmp_path, inputs, projected):
    s, indptr, indices, n_features, argv = inputs
    out_dir = tmp_path / "out"
    cli.main(["-o", str(out_dir), "--rescore", "weighted_jaccard", "--rescore-candidates", str(KP), "--refine",
              "weighted_jaccard", "--refine-fan", "3", "--refine-reverse", "--symmetrize", "mutual"] + argv)
    values = cli.sparse_weights(s["counts"], n_features, "weighted_jaccard")[indices]
    with ctx.rescore_rows(indptr, indices, values, n_features, metric="weighted_jaccard") as held:
        lists = held.knn(projected[KP][0], K)
        refined = held.refine(lists, K, fan=3, reverse=True)
    want = tmp_path / "want.tsv"
    _written(want, ctx.graph_symmetrize(refined, "mutual"), s)
    assert open(out_dir / "overlaps.tsv", "rb").read() == want.read_bytes()


@pytest.mark.parametrize("flags, message", [
    (["--refine", "jaccard", "--radius", "0.2"], "--refine refines k-NN lists: it does not run with --radius"),
    (["--refine", "jaccard", "--no-projection"], "--refine refines the projected search's lists"),
    (["--refine", "jaccard", "--devices", "0,1"], "--refine runs on one GPU"),
    (["--refine", "jaccard", "--rescore", "cosine"], "the two metrics must be the same"),
    (["--refine", "jaccard", "--refine-fan", "0"], r"--refine-fan must be in \[1, 128\], got 0"),
    (["--refine", "jaccard", "--refine-fan", "129"], r"--refine-fan must be in \[1, 128\], got 129"),
    (["--refine", "jaccard", "--refine-rounds", "0"], "--refine-rounds must be at least 1"),
    (["--refine-fan", "5"], "--refine-fan needs --refine"),
    (["--refine-rounds", "2"], "--refine-rounds needs --refine"),
    (["--refine-reverse"], "--refine-reverse needs --refine"),
])
def test_refused_combinations_exit_with_their_message(tmp_path, inputs, flags, message):
    argv = inputs[-1]
    with pytest.raises(SystemExit, match=message):
        cli.main(["-o", str(tmp_path / "out")] + flags + argv)
    assert not (tmp_path / "out" / "overlaps.tsv").exists()
