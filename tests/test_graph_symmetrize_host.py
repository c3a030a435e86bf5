"""fedrann_amd.graph.symmetrize_rows (the numpy model of fdr_graph_symmetrize) against a dict-of-pairs brute force and
against the identities of the three modes; the argument checks of Context.graph_symmetrize, which come before the
library; the ABI names; the command line's --symmetrize.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _graph_rows as gr
from _radius_model import same
from conftest import ROOT
from fedrann_amd import __main__ as cli
from fedrann_amd import _lib
from fedrann_amd.graph import as_ragged, symmetrize_rows

SIZES = (1, 2, 65, 300)


@pytest.fixture(scope="module", params=SIZES)
def graph(request):
    n = request.param
    return gr.drawn(n, seed=100 + n)


@pytest.mark.parametrize("mode", gr.MODES)
def test_model_is_the_brute_force(graph, mode):
    got = symmetrize_rows(*graph, mode)
    same(got, gr.brute(graph, mode))
    key = (gr.bits(got[2]).astype(np.uint64) << np.uint64(32)) | got[1].astype(np.uint64)
    rows = np.repeat(np.arange(got[0].size - 1), np.diff(got[0]))
    inside = rows[1:] == rows[:-1]
    assert np.all(key[1:][inside] > key[:-1][inside])  # every row strictly ascending by key


def test_identities(graph):
    union, mutual, transpose = (symmetrize_rows(*graph, m) for m in gr.MODES)
    same(symmetrize_rows(*transpose, "transpose"), graph)  # (the graph's rows are sorted)
    same(symmetrize_rows(*union, "transpose"), union)
    same(symmetrize_rows(*mutual, "transpose"), mutual)
    assert gr.pairs(mutual) <= gr.pairs(graph) <= gr.pairs(union)
    assert union[1].size + mutual[1].size == 2 * graph[1].size  # (self entries included)
    for sym in (union, mutual):  # a symmetric graph comes back unchanged
        same(symmetrize_rows(*sym, "union"), sym)
        same(symmetrize_rows(*sym, "mutual"), sym)


def test_the_drawn_graphs_cover_the_cases():
    g = gr.drawn(300, seed=400)
    lens = np.diff(g[0])
    assert {0, 1, 63, 64, 65, 300} <= set(lens.tolist())
    assert np.any(g[1] == np.repeat(np.arange(300), lens))  # self entries
    assert 0 < symmetrize_rows(*g, "mutual")[1].size < g[1].size  # one-way and two-way pairs


def test_asymmetric_distances_take_the_smaller_bits_and_transpose_the_listers():
    g = gr.asymmetric()
    for mode in gr.MODES:
        same(symmetrize_rows(*g, mode), gr.brute(g, mode))
    tiny = gr.TINY
    union, mutual, transpose = (symmetrize_rows(*g, m) for m in gr.MODES)

    def row(res, r):
        return list(zip(res[1][res[0][r]:res[0][r + 1]].tolist(), res[2][res[0][r]:res[0][r + 1]].tolist()))
    assert row(union, 0) == [(0, 0.0), (3, 0.0), (1, 0.25)] and row(mutual, 0) == row(union, 0)
    assert row(union, 3) == [(0, 0.0)] and row(mutual, 3) == [(0, 0.0)]
    assert row(union, 1) == [(2, 0.125), (0, 0.25)] and row(mutual, 1) == row(union, 1)
    assert row(union, 2) == [(1, 0.125), (2, 0.375), (4, 0.5)] and row(mutual, 2) == [(1, 0.125), (2, 0.375)]
    assert row(union, 4) == [(2, 0.5)] and row(mutual, 4) == []
    assert row(transpose, 0) == [(0, 0.0), (3, 0.0), (1, 0.25)]
    assert row(transpose, 3) == [(0, tiny)] and row(transpose, 1) == [(2, 0.125), (0, 0.5)]
    assert row(transpose, 2) == [(2, 0.375), (1, 0.75)] and row(transpose, 4) == [(2, 0.5)]
    assert gr.bits(np.float32(tiny)) == 1


@pytest.mark.parametrize("mode", gr.MODES)
def test_unsorted_rows_give_the_result_of_the_sorted_rows(mode):
    for n in SIZES:
        shuffled = gr.drawn(n, seed=200 + n, shuffled=True)
        ordered = gr.sort_rows(shuffled)
        assert n < 65 or not np.array_equal(shuffled[1], ordered[1])
        same(symmetrize_rows(*shuffled, mode), symmetrize_rows(*ordered, mode))


def test_as_ragged_takes_both_forms():
    idx = np.array([[1, 0], [0, 1], [2, 0]], np.int32)
    dist = np.array([[0.5, 0.0], [0.5, 0.25], [0.0, 0.25]], np.float32)
    ip, ix, ds = as_ragged((idx, dist))
    assert ip.tolist() == [0, 2, 4, 6] and ip.dtype == np.int64
    assert ix.tolist() == idx.ravel().tolist() and ds.tolist() == dist.ravel().tolist()
    same(as_ragged((ip, ix, ds)), (ip, ix, ds))
    same(symmetrize_rows(ip, ix, ds, "union"), gr.brute((ip, ix, ds), "union"))
    assert as_ragged((np.zeros((4, 0), np.int32), np.zeros((4, 0), np.float32)))[0].tolist() == [0] * 5


# ---- the model's refusals ----------------------------------------------------------------------------------------------
def _edited(graph, fn):
    out = tuple(a.copy() for a in graph)
    fn(*out)
    return out


def test_model_refuses_the_three_rules_with_the_smallest_row_and_rule():
    good = gr.drawn(65, seed=7, shuffled=True, lengths=(5, 63, 64, 65))
    ip = good[0]

    def index(r, j, v):
        return lambda _, ix, ds: ix.__setitem__(int(ip[r]) + j, v)

    def distance(r, j, v):
        return lambda _, ix, ds: ds.__setitem__(int(ip[r]) + j, v)

    def twice(r, a, b):
        return lambda _, ix, ds: ix.__setitem__(int(ip[r]) + b, ix[int(ip[r]) + a])
    for mode in gr.MODES:
        for fn, words in ((index(0, 0, -1), "row 0: an index outside"), (index(64, 4, 65), "row 64: an index outside"),
                          (distance(3, 1, -0.5), "row 3: a distance that is negative or NaN"),
                          (distance(3, 1, -0.0), "row 3: a distance that is negative or NaN"),
                          (distance(64, 4, np.nan), "row 64: a distance that is negative or NaN"),
                          (twice(9, 0, 4), "row 9: an index listed twice")):
            with pytest.raises(ValueError, match=words):
                symmetrize_rows(*_edited(good, fn), mode)
    several = _edited(_edited(_edited(good, twice(5, 0, 2)), distance(5, 1, np.nan)), index(40, 0, -2))
    with pytest.raises(ValueError, match="row 5: a distance"):  # (row 5 before row 40, rule 2 before rule 3)
        symmetrize_rows(*several, "union")
    with pytest.raises(ValueError, match="row 5: an index outside"):
        symmetrize_rows(*_edited(several, index(5, 3, 99)), "mutual")
    with pytest.raises(ValueError, match="mode must be one of"):
        symmetrize_rows(*good, "both")
    with pytest.raises(ValueError, match="at least one row"):
        symmetrize_rows(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), "union")


# ---- Context.graph_symmetrize: the checks come before the library ------------------------------------------------------------
class _NoLibrary(_lib.Context):
    """A context whose library must never be reached."""

    def __init__(self):
        self._h = None

    @property
    def _L(self):
        raise AssertionError("the library was called")


def test_good_arguments_pass_the_checks():
    g = gr.drawn(65, seed=3)
    code, n, ip, ix, ds = _lib.check_graph_symmetrize(g, "mutual", 1)
    assert (code, n) == (1, 65) and ip is g[0] and ix is g[1] and ds is g[2]
    assert [_lib.check_graph_symmetrize(g, m)[0] for m in gr.MODES] == [0, 1, 2]
    rect = (np.zeros((3, 2), np.int32), np.zeros((3, 2), np.float32))
    assert _lib.check_graph_symmetrize(rect)[:2] == (0, 3)


def test_bad_arguments_raise_before_the_library_is_called():
    c = _NoLibrary()
    ip, ix, ds = gr.drawn(65, seed=3)
    for bad in (np.array([1, 2, 3], np.int64), np.array([0, 2, 1], np.int64), np.array([0, -1, 3], np.int64)):
        with pytest.raises(ValueError, match="start at 0 and never decrease"):
            c.graph_symmetrize((bad, ix[:3].copy(), ds[:3].copy()))
    with pytest.raises(ValueError, match="entries indptr states"):
        c.graph_symmetrize((ip, ix[:-1].copy(), ds))
    with pytest.raises(ValueError, match="indptr must be int64"):
        c.graph_symmetrize((ip.astype(np.int32), ix, ds))
    with pytest.raises(ValueError, match="idx must be int32"):
        c.graph_symmetrize((ip, ix.astype(np.int64), ds))
    with pytest.raises(ValueError, match="dist float32"):
        c.graph_symmetrize((ip, ix, ds.astype(np.float64)))
    with pytest.raises(ValueError, match="one shape"):
        c.graph_symmetrize((np.zeros((3, 2), np.int32), np.zeros((3, 3), np.float32)))
    with pytest.raises(ValueError, match="one shape"):
        c.graph_symmetrize((ix, ds))
    with pytest.raises(ValueError, match="three 1-D arrays"):
        c.graph_symmetrize((ip, ix.reshape(1, -1), ds.reshape(1, -1)))
    for bad in ((ip,), (ip, ix, ds, ds), 7, (ip.tolist(), ix, ds)):
        with pytest.raises(ValueError, match="a graph is"):
            c.graph_symmetrize(bad)
    for mode in ("both", 0, None, "Union"):
        with pytest.raises(ValueError, match="mode must be one of"):
            c.graph_symmetrize((ip, ix, ds), mode=mode)
    for cap in (0, 2 ** 31, 2.0, True):
        with pytest.raises(ValueError, match="max_entries"):
            c.graph_symmetrize((ip, ix, ds), max_entries=cap)
    with pytest.raises(ValueError, match="1 <= n < 2\\^31"):
        c.graph_symmetrize((np.zeros(1, np.int64), ix[:0].copy(), ds[:0].copy()))
    with pytest.raises(ValueError, match="1 <= n < 2\\^31"):
        c.graph_symmetrize((np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32)))


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_the_three_names_are_in_the_header_and_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "fedrann_hip.h")).read()
    L = _lib.load_library()
    for name, args in (("fdr_graph_symmetrize", 8), ("fdr_graph_symmetrize_fetch", 4), ("fdr_graph_free", 1)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m and name in _lib.SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 1 + m.group(1).count(",") == args
    for name, value in (("UNION", 0), ("MUTUAL", 1), ("TRANSPOSE", 2)):
        assert re.search(r"#define FDR_GRAPH_%s %d\b" % (name, value), hdr)
    from fedrann_amd import graph
    assert graph.MODES == {"union": 0, "mutual": 1, "transpose": 2}
    ip = np.zeros(2, np.int64)
    assert L.fdr_graph_symmetrize(None, 0, 1, ip.ctypes.data, None, None, 1, ip.ctypes.data) == -1  # FDR_E_ARG
    assert b"null context" in L.fdr_last_error()
    assert L.fdr_graph_symmetrize_fetch(None, 0, None, None) == -1 and L.fdr_graph_free(None) == -1


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE = ["--feature-matrix", "x.npz", "--kmer-counts", "c.npy"]


@pytest.mark.parametrize("extra", [[], ["--no-projection"], ["--radius", "0.5"], ["--rescore", "jaccard"],
                                   ["--no-projection", "--no-projection-radius", "0.5", "--sparse-shard", "targets"]])
def test_symmetrize_over_several_devices_is_refused_before_any_work(tmp_path, extra):
    out_dir = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        cli.main(["-o", str(out_dir), "--symmetrize", "union", "--devices", "0,1"] + BASE + extra)
    assert not os.path.exists(out_dir)  # refused before the output directory is made
    if not extra:
        assert all(w in str(e.value) for w in ("--symmetrize", "one GPU", "--devices", "reverse entry"))


def test_a_bad_choice_is_refused_and_the_flag_is_optional(capsys):
    for bad in ("transpose", "both", ""):
        with pytest.raises(SystemExit):
            cli.parse_command_line_arguments(["-o", "x", "--symmetrize", bad] + BASE)
    assert "--symmetrize" in capsys.readouterr().err
    plain = cli.parse_command_line_arguments(["-o", "x"] + BASE)
    assert plain.symmetrize is None
    cli.check_symmetrize(plain)
    for mode in ("union", "mutual"):
        flagged = cli.parse_command_line_arguments(["-o", "x", "--symmetrize", mode, "--devices", "0"] + BASE)
        assert flagged.symmetrize == mode
        cli.check_symmetrize(flagged)  # (one device: fine)
        a, b = dict(vars(plain)), dict(vars(flagged))
        assert a.pop("symmetrize") is None and b.pop("symmetrize") == mode and b.pop("devices") == "0"
        assert a.pop("devices") is None and a == b  # every other default as it was
    text = cli.build_parser().format_help()
    assert "--symmetrize {union,mutual}" in text and "collect their row blocks on the host" in " ".join(text.split())
    assert "Refused over several --devices" in " ".join(text.split())
