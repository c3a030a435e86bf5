"""`--no-projection-radius R`: overlaps.tsv of the command line equals, byte for byte, the file written in one piece from
SparseIndex.radius_search on the same rows through the ragged writer; the flag's refusals come before any work."""
import os

import numpy as np
import pytest

from fedrann_amd import __main__ as cli
from fedrann_amd import _lib
from fedrann_amd import feature_extraction as fx
from fedrann_amd.synth import synth

pytestmark = pytest.mark.gpu


def _inputs(tmp_path):
    """The feature-matrix input of test_gpu_cli.test_cli_from_feature_matrix_npz."""
    s = synth(1500, seed=9, m=60, doubling=True)
    npz = tmp_path / "feature_matrix.npz"
    fx.save_feature_matrix_npz(str(npz), s["indptr"], s["indices"], s["n_features"])
    counts = tmp_path / "counts.npy"
    np.save(counts, s["counts"])
    names = tmp_path / "names.txt"
    with open(names, "w") as f:
        for n, st in zip(s["names"], s["strands"]):
            f.write("%s\t%d\n" % (n, st))
    return s, ["--feature-matrix", str(npz), "--kmer-counts", str(counts), "--read-names", str(names)]


def test_cli_radius_equals_the_search_written_in_one_piece(ctx, tmp_path, monkeypatch):
    s, inputs = _inputs(tmp_path)
    indptr = np.ascontiguousarray(s["indptr"], dtype=np.int64)
    indices = np.ascontiguousarray(s["indices"], dtype=np.int32)
    n = indptr.size - 1
    with ctx.sparse_index(indptr, indices, None, s["n_features"], metric="jaccard") as index:
        res = index.radius_search(0.9)
    # The command line's block loop: several appended blocks, the last one short, and a cap on the hits of one device
    # call that every read fits under but the fullest block does not, so the wrapper cuts that block by its counts.
    block = 700
    blocks = [(lo, min(n, lo + block)) for lo in range(0, n, block)]
    assert len(blocks) >= 3 and blocks[-1][1] - blocks[-1][0] < block
    totals = [int(res[0][hi] - res[0][lo]) for lo, hi in blocks]
    cap = max(int(np.diff(res[0]).max()), max(totals) // 3)
    assert cap < max(totals)
    monkeypatch.setattr(cli, "RADIUS_BLOCK_ROWS", block)
    monkeypatch.setattr(cli, "RADIUS_MAX_HITS", cap)
    searches, raw = [], []
    search, call = _lib.SparseIndex.radius_search, _lib.SparseIndex._radius_call

    def counted_search(self, radius, lo=0, hi=None, max_hits=1 << 26):
        searches.append((lo, hi, max_hits))
        return search(self, radius, lo, hi, max_hits=max_hits)

    def counted_call(self, what, fn, nq, max_hits):
        raw.append(nq)
        return call(self, what, fn, nq, max_hits)
    monkeypatch.setattr(_lib.SparseIndex, "radius_search", counted_search)
    monkeypatch.setattr(_lib.SparseIndex, "_radius_call", counted_call)
    out_dir = tmp_path / "out"
    cli.main(["-o", str(out_dir), "--no-projection", "--no-projection-metric", "jaccard", "--no-projection-radius",
              "0.9", "--nndescent-n-neighbors", "7"] + inputs)
    monkeypatch.undo()
    assert searches == [(lo, hi, cap) for lo, hi in blocks]
    over = sum(t > cap for t in totals)
    assert over >= 1 and len(raw) >= len(blocks) + 2 * over  # (a block over the cap: its counts, then >= 2 pieces)
    got = open(out_dir / "overlaps.tsv", "rb").read()
    off, buf8 = _lib.pack_names(s["names"])
    want = tmp_path / "want.tsv"
    lines = _lib.overlaps_write_csr(str(want), *res, off, buf8, np.asarray(s["strands"], np.uint8))
    assert got == want.read_bytes()
    rows = got.decode().splitlines()[1:]
    assert len(rows) == lines >= 1 and lines == res[0][-1] - (indptr.size - 1)  # (every row's self entry is dropped)
    dist = np.array([float(r.split("\t")[5]) for r in rows])
    assert dist.max() <= 0.9
    assert np.unique(np.diff(res[0])).size > 3  # ragged: reads differ in their number of neighbours
    assert "--nndescent-n-neighbors (7) are ignored" in open(out_dir / "fedrann.log").read()


@pytest.mark.parametrize("extra,words", [
    (["--no-projection", "--no-projection-radius", "1.0"], ("[0, 1)",)),
    (["--no-projection", "--no-projection-radius", "-0.5"], ("[0, 1)",)),
    (["--no-projection", "--no-projection-radius", "nan"], ("[0, 1)",)),
    (["--no-projection-radius", "0.5"], ("needs --no-projection",)),
    (["--no-projection", "--no-projection-radius", "0.5", "--devices", "0,0", "--sparse-shard", "queries"],
     ("one GPU", "--devices")),
    (["--no-projection", "--no-projection-radius", "0.5", "--devices", "0,0"], ("one GPU", "--devices")),
])
def test_cli_radius_refusals_come_before_any_work(tmp_path, extra, words):
    out_dir = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        cli.main(["-o", str(out_dir), "--feature-matrix", str(tmp_path / "none.npz"), "--kmer-counts",
                  str(tmp_path / "none.npy")] + extra)
    assert all(w in str(e.value) for w in words), e.value
    assert not os.path.exists(out_dir)  # refused before the output directory is made
