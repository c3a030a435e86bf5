"""`--radius R` in the default, projected mode: overlaps.tsv of the command line equals, byte for byte, the file the
ragged writer makes of the ORACLE's result (the oracle's projection, embedding and ranking of all rows, cut at R) on the
inputs of test_gpu_cli.test_cli_from_feature_matrix_npz."""
import numpy as np
import pytest

import _dense_radius_model as dmodel
import _radius_model as rmodel
from fedrann_amd import __main__ as cli
from fedrann_amd import _lib
from fedrann_amd import feature_extraction as fx
from fedrann_amd.synth import synth

pytestmark = pytest.mark.gpu


def test_cli_radius_equals_the_oracle_written_in_one_piece(tmp_path, oracle, monkeypatch):
    s = synth(1500, seed=9, m=60, doubling=True)
    npz = tmp_path / "feature_matrix.npz"
    fx.save_feature_matrix_npz(str(npz), s["indptr"], s["indices"], s["n_features"])
    counts = tmp_path / "counts.npy"
    np.save(counts, s["counts"])
    names = tmp_path / "names.txt"
    with open(names, "w") as f:
        for n, st in zip(s["names"], s["strands"]):
            f.write("%s\t%d\n" % (n, st))
    P = oracle.precompute_matrix(s["counts"], 128)
    E = oracle.embed(s["indptr"], s["indices"], P, s["n_features"], 128)
    n = E.shape[0]
    idx, dist = dmodel.ranked(oracle, E)
    r = float(np.sort(dist[:, 8])[n // 2])  # the median distance of the ninth entry: rows with fewer and with more hits
    res = rmodel.cut_ranked(idx, dist, np.float32(r))
    # several appended blocks, the last one short, and a cap that the fullest block's candidates pass
    block = 700
    blocks = [(lo, min(n, lo + block)) for lo in range(0, n, block)]
    assert len(blocks) >= 3 and blocks[-1][1] - blocks[-1][0] < block
    totals = [int(res[0][hi] - res[0][lo]) for lo, hi in blocks]
    cap = max(int(np.diff(res[0]).max()) * 4, max(totals) // 3)
    assert cap < max(totals)  # (the candidates are no fewer than the hits)
    monkeypatch.setattr(cli, "RADIUS_BLOCK_ROWS", block)
    monkeypatch.setattr(cli, "RADIUS_MAX_HITS", cap)
    searches = []
    search = _lib.DenseIndex.radius_search

    def counted_search(self, radius, lo=0, hi=None, max_hits=1 << 26):
        searches.append((lo, hi, max_hits))
        return search(self, radius, lo, hi, max_hits=max_hits)
    monkeypatch.setattr(_lib.DenseIndex, "radius_search", counted_search)
    out_dir = tmp_path / "out"
    cli.main(["-o", str(out_dir), "-n", "128", "--radius", repr(r), "--nndescent-n-neighbors", "7", "--feature-matrix",
              str(npz), "--kmer-counts", str(counts), "--read-names", str(names)])
    monkeypatch.undo()
    assert searches == [(lo, hi, cap) for lo, hi in blocks]
    got = open(out_dir / "overlaps.tsv", "rb").read()
    off, buf8 = _lib.pack_names(s["names"])
    want = tmp_path / "want.tsv"
    lines = _lib.overlaps_write_csr(str(want), *res, off, buf8, np.asarray(s["strands"], np.uint8))
    assert got == want.read_bytes()
    assert lines == res[0][-1] - n >= 1  # (every row's self entry is dropped)
    assert np.unique(np.diff(res[0])).size > 3  # ragged: reads differ in their number of neighbours
    assert "--radius: --nndescent-n-neighbors (7) is ignored" in open(out_dir / "fedrann.log").read()
