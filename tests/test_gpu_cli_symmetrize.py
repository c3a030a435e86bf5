"""`--symmetrize union|mutual` on one GPU, in the default projected mode, with --no-projection (Jaccard) and with
--radius: overlaps.tsv equals, byte for byte, the file overlaps_write_csr makes of graph.symmetrize_rows applied to
the rows the same mode writes without the flag.

Those rows are read back at the writer's door (the arrays the unflagged run hands to overlaps_write /
overlaps_write_csr), not from its file: the file leaves out a read's entry for itself, whose distance bits decide its
place in the symmetrised row and so the neighbor_rank of the entries behind it."""
import numpy as np
import pytest

from fedrann_amd import __main__ as cli
from fedrann_amd import _lib
from fedrann_amd import feature_extraction as fx
from fedrann_amd.graph import as_ragged, symmetrize_rows
from fedrann_amd.synth import synth

pytestmark = pytest.mark.gpu

SEARCHES = {
    "projected": ["--nndescent-n-neighbors", "20"],
    "jaccard": ["--nndescent-n-neighbors", "20", "--no-projection", "--no-projection-metric", "jaccard"],
    "radius": ["--radius", "0.6"],
}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("symmetrize_cli")
    s = synth(300, seed=9, m=60, doubling=True)
    npz = tmp / "feature_matrix.npz"
    fx.save_feature_matrix_npz(str(npz), s["indptr"], s["indices"], s["n_features"])
    counts = tmp / "counts.npy"
    np.save(counts, s["counts"])
    names = tmp / "names.txt"
    with open(names, "w") as f:
        for n, st in zip(s["names"], s["strands"]):
            f.write("%s\t%d\n" % (n, st))
    return s, ["-n", "128", "--feature-matrix", str(npz), "--kmer-counts", str(counts), "--read-names", str(names)]


class _Door:
    """What a run hands to the two writers and to graph_symmetrize, the calls themselves untouched; run() starts a
    new record."""

    def __init__(self, monkeypatch):
        self.rect, self.ragged, self.symmetrized = [], [], []
        write, write_csr, sym = _lib.overlaps_write, _lib.overlaps_write_csr, _lib.Context.graph_symmetrize

        def spy_write(path, idx, dist, *a, **kw):
            self.rect.append((np.array(idx), np.array(dist)))
            return write(path, idx, dist, *a, **kw)

        def spy_write_csr(path, indptr, idx, dist, *a, **kw):
            self.ragged.append((np.array(indptr), np.array(idx), np.array(dist), kw.get("row0", 0)))
            return write_csr(path, indptr, idx, dist, *a, **kw)

        def spy_sym(ctx, graph, mode="union", **kw):
            self.symmetrized.append(mode)
            return sym(ctx, graph, mode, **kw)
        monkeypatch.setattr(_lib, "overlaps_write", spy_write)
        monkeypatch.setattr(_lib, "overlaps_write_csr", spy_write_csr)
        monkeypatch.setattr(_lib.Context, "graph_symmetrize", spy_sym)

    def run(self, argv):
        self.rect, self.ragged, self.symmetrized = [], [], []
        cli.main(argv)
        return self

    def graph(self):
        """the rows of the run's one rectangular write, or of its ragged writes in row order"""
        if self.rect:
            assert len(self.rect) == 1 and not self.ragged
            idx, dist = self.rect[0]
            return as_ragged((np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(dist, np.float32)))
        assert [b[3] for b in self.ragged] == list(np.cumsum([0] + [b[0].size - 1 for b in self.ragged[:-1]]))
        starts = np.cumsum([0] + [int(b[0][-1]) for b in self.ragged[:-1]])
        indptr = np.concatenate([np.zeros(1, np.int64)] + [b[0][1:] + s for b, s in zip(self.ragged, starts)])
        return indptr, np.concatenate([b[1] for b in self.ragged]), np.concatenate([b[2] for b in self.ragged])


@pytest.mark.parametrize("search", sorted(SEARCHES))
def test_cli_equals_the_model_on_the_unflagged_rows(tmp_path, monkeypatch, inputs, search):
    s, argv = inputs
    argv = argv + SEARCHES[search]
    door = _Door(monkeypatch).run(["-o", str(tmp_path / "plain")] + argv)
    graph = door.graph()
    writes = len(door.rect), len(door.ragged)
    assert not door.symmetrized and graph[0].size - 1 == 600 and graph[1].size > 600
    plain = open(tmp_path / "plain" / "overlaps.tsv", "rb").read()
    # without the flag: the same writer, the same bytes, run after run
    door.run(["-o", str(tmp_path / "again")] + argv)
    assert not door.symmetrized and (len(door.rect), len(door.ragged)) == writes
    assert open(tmp_path / "again" / "overlaps.tsv", "rb").read() == plain and plain.count(b"\n") > 600
    name_off, names = _lib.pack_names(s["names"])
    strands = np.asarray(s["strands"], np.uint8)
    files = {}
    for mode in ("union", "mutual"):
        out_dir = tmp_path / mode
        door.run(["-o", str(out_dir), "--symmetrize", mode] + argv)
        assert door.symmetrized == [mode] and not door.rect and len(door.ragged) == 1  # written once
        want = tmp_path / (mode + ".tsv")
        lines = _lib.overlaps_write_csr(str(want), *symmetrize_rows(*graph, mode), name_off, names, strands)
        files[mode] = open(out_dir / "overlaps.tsv", "rb").read()
        assert lines > 0 and files[mode] == want.read_bytes()
        assert "--symmetrize %s:" % mode in open(out_dir / "fedrann.log").read()
    assert files["mutual"].count(b"\n") <= plain.count(b"\n") <= files["union"].count(b"\n")
    if search != "radius":  # (k nearest is a one-way relation; within a radius is not)
        assert files["mutual"].count(b"\n") < plain.count(b"\n") < files["union"].count(b"\n")
