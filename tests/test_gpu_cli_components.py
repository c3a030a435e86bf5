"""`--components union|mutual [--components-distance D]` on one GPU, in the default projected mode, with --no-projection
(Jaccard) and with --radius: components.tsv equals the file made from graph.component_labels of the rows the same mode
writes without the flag, overlaps.tsv is the unflagged run's byte for byte, and with --symmetrize the components are
still those of the rows as searched.

Those rows are read back at the writer's door (the arrays the unflagged run hands to overlaps_write /
overlaps_write_csr), not from its file: the file leaves out a read's entry for itself.  The refusals need no GPU."""
import numpy as np
import pytest

from fedrann_amd import __main__ as cli
from fedrann_amd import _lib
from fedrann_amd import feature_extraction as fx
from fedrann_amd.graph import as_ragged, component_labels, symmetrize_rows
from fedrann_amd.synth import synth

SEARCHES = {
    "projected": ["--nndescent-n-neighbors", "20"],
    "jaccard": ["--nndescent-n-neighbors", "20", "--no-projection", "--no-projection-metric", "jaccard"],
    "radius": ["--radius", "0.6"],
}
HEADER = "read_name\torientation\tcomponent\tcomponent_size\n"


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("components_cli")
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
    """What a run hands to the two writers, and the modes it asks graph_components and graph_symmetrize for, the calls
    themselves untouched; run() starts a new record."""

    def __init__(self, monkeypatch):
        self.run_argv = None
        write, write_csr = _lib.overlaps_write, _lib.overlaps_write_csr
        sym, comp = _lib.Context.graph_symmetrize, _lib.Context.graph_components

        def spy_write(path, idx, dist, *a, **kw):
            self.rect.append((np.array(idx), np.array(dist)))
            return write(path, idx, dist, *a, **kw)

        def spy_write_csr(path, indptr, idx, dist, *a, **kw):
            self.ragged.append((np.array(indptr), np.array(idx), np.array(dist), kw.get("row0", 0)))
            return write_csr(path, indptr, idx, dist, *a, **kw)

        def spy_sym(ctx, graph, mode="union", **kw):
            self.symmetrized.append(mode)
            return sym(ctx, graph, mode, **kw)

        def spy_comp(ctx, graph, mode="union", max_distance=None):
            self.labelled.append((mode, max_distance, as_ragged(graph)))
            return comp(ctx, graph, mode, max_distance)
        monkeypatch.setattr(_lib, "overlaps_write", spy_write)
        monkeypatch.setattr(_lib, "overlaps_write_csr", spy_write_csr)
        monkeypatch.setattr(_lib.Context, "graph_symmetrize", spy_sym)
        monkeypatch.setattr(_lib.Context, "graph_components", spy_comp)

    def run(self, argv):
        self.rect, self.ragged, self.symmetrized, self.labelled = [], [], [], []
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


def _file_of(s, labels, sizes):
    lines = [HEADER]
    for r, (name, strand) in enumerate(zip(s["names"], s["strands"])):
        lines.append("%s\t%s\t%d\t%d\n" % (name, "+-"[int(strand)], labels[r], sizes[labels[r]]))
    return "".join(lines)


@pytest.mark.gpu
@pytest.mark.parametrize("search", sorted(SEARCHES))
def test_cli_writes_the_models_components_of_the_unflagged_rows(tmp_path, monkeypatch, inputs, search):
    s, argv = inputs
    argv = argv + SEARCHES[search]
    door = _Door(monkeypatch).run(["-o", str(tmp_path / "plain")] + argv)
    graph = door.graph()
    writes = len(door.rect), len(door.ragged)
    assert not door.labelled and graph[0].size - 1 == 600 and graph[1].size > 600
    assert not (tmp_path / "plain" / "components.tsv").exists()
    plain = open(tmp_path / "plain" / "overlaps.tsv", "rb").read()
    cut = float(np.quantile(graph[2][graph[2] > 0], 0.1))  # a tenth of the pairs: the two strands' components fall apart
    seen = set()
    for mode in ("union", "mutual"):
        for bound in (None, cut):
            out_dir = tmp_path / ("%s_%s" % (mode, bound))
            flags = ["--components", mode] + ([] if bound is None else ["--components-distance", repr(bound)])
            door.run(["-o", str(out_dir)] + flags + argv)
            assert not door.symmetrized and (len(door.rect), len(door.ragged)) == writes  # the same writer ...
            assert open(out_dir / "overlaps.tsv", "rb").read() == plain  # ... and the same bytes
            assert [(m, b) for m, b, _ in door.labelled] == [(mode, bound)]
            assert all(np.array_equal(a, b) for a, b in zip(door.labelled[0][2], graph))  # the rows as searched
            labels, sizes = component_labels(*graph, mode, bound)
            got = open(out_dir / "components.tsv").read()
            assert got == _file_of(s, labels, sizes) and got.count("\n") == 601
            log = open(out_dir / "fedrann.log").read()
            assert "--components %s: %d components of 600 rows, the largest of %d, %d singletons" % (
                mode, sizes.size, sizes.max(), np.sum(sizes == 1)) in log
            seen.add(got)
    assert len(seen) >= 2  # the flags show
    # with --symmetrize: the symmetrised overlaps, and the components of the rows as searched
    out_dir = tmp_path / "both"
    door.run(["-o", str(out_dir), "--symmetrize", "mutual", "--components", "mutual"] + argv)
    assert door.symmetrized == ["mutual"] and not door.rect and len(door.ragged) == 1
    assert all(np.array_equal(a, b) for a, b in zip(door.labelled[0][2], graph))
    name_off, names = _lib.pack_names(s["names"])
    want = tmp_path / "mutual.tsv"
    _lib.overlaps_write_csr(str(want), *symmetrize_rows(*graph, "mutual"), name_off, names,
                            np.asarray(s["strands"], np.uint8))
    assert open(out_dir / "overlaps.tsv", "rb").read() == want.read_bytes()
    assert open(out_dir / "components.tsv").read() == _file_of(s, *component_labels(*graph, "mutual"))


def test_refusals_before_any_work(tmp_path, inputs):
    _, argv = inputs
    out = ["-o", str(tmp_path / "never")]
    with pytest.raises(SystemExit, match="--components-distance needs --components"):
        cli.main(out + argv + ["--components-distance", "0.5"])
    for bad in ("-0.5", "nan", "-inf", "-0.0"):
        with pytest.raises(SystemExit, match="--components-distance must be a distance >= 0"):
            cli.main(out + argv + ["--components", "union", "--components-distance=" + bad])
    with pytest.raises(SystemExit, match="--components runs on one GPU: over --devices a rank holds only its own rows' "
                                         "lists, and a reverse entry can come from any row"):
        cli.main(out + argv + ["--components", "mutual", "--devices", "0,1"])
    with pytest.raises(SystemExit):  # argparse: transpose is no choice
        cli.main(out + argv + ["--components", "transpose"])
    assert not (tmp_path / "never").exists()
