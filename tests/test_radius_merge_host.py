"""The merge of the ranks' ragged radius rows without a GPU: distributed.merge_sparse_radius against the radius model
(tests/_radius_model.rows_within) on the rows of the three-rank test, shard by shard; the entry point in the header, the
bindings and the library; the argument checks of Context.radius_merge, which raise before the library is called; the
command line's checks of --no-projection-radius over --devices."""
import ctypes
import os
import re

import numpy as np
import pytest

import _radius_model as rmodel
from _gpu_sparse_sharded_worker import sharded_rows, values_of
from conftest import ROOT
from fedrann_amd import __main__ as cli
from fedrann_amd import _lib
from fedrann_amd.distributed import merge_sparse_radius, sparse_radius_offsets

R, WORLD = 1500, 3
RADII = (0.0, 0.5, 0.9)


@pytest.fixture(scope="module")
def rows():
    indptr, indices, F, weights, blocks = sharded_rows(R, WORLD)
    return indptr, indices, F, weights, blocks


@pytest.fixture(scope="module")
def matrices(rows):
    """metric -> float32 [n, n]: every row against every row, computed once."""
    indptr, indices, F, weights, _ = rows
    out = {}
    for metric in ("jaccard", "weighted_jaccard"):
        csr = (indptr, indices, values_of(metric, weights, indices))
        out[metric] = rmodel.distances(metric, csr, csr, F)
    return out


def _shard_parts(D, blocks, r):
    parts = []
    for lo, hi in blocks:
        ip, ix, ds = rmodel.rows_within(D[:, lo:hi], r)
        parts.append((ip, ix + np.int32(lo), ds))
    return parts


# ---- the model of the kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jaccard", "weighted_jaccard"])
@pytest.mark.parametrize("r", RADII)
def test_the_merge_of_the_shards_rows_is_the_whole_result(rows, matrices, metric, r):
    blocks = rows[4]
    D = matrices[metric]
    want = rmodel.rows_within(D, r)
    parts = _shard_parts(D, blocks, r)
    assert sum(int(p[0][-1]) for p in parts) == int(want[0][-1])
    assert np.array_equal(sum(np.diff(p[0]) for p in parts), np.diff(want[0]))  # (row by row)
    rmodel.same(merge_sparse_radius(parts), want)
    rmodel.same(merge_sparse_radius(parts[::-1]), want)  # (distinct indices: the order of the parts is nothing)
    rmodel.same(merge_sparse_radius([parts[1], parts[2], parts[0]]), want)


def test_the_rows_are_what_the_test_is_about(rows, matrices):
    indptr, indices, F, weights, blocks = rows
    D = matrices["jaccard"]
    assert D.shape == (3000, 3000) and blocks == [(0, 1024), (1024, 2048), (2048, 3000)]
    whole = {r: rmodel.rows_within(D, r) for r in (0.5, 0.9)}
    assert int(whole[0.5][0][-1]) == 19_780 and int(whole[0.9][0][-1]) == 142_970
    assert int((np.diff(whole[0.9][0]) > 64).sum()) == 337  # (rows longer than a wave)
    parts = _shard_parts(D, blocks, 0.9)
    from_all = np.all([np.diff(p[0]) > 0 for p in parts], axis=0)
    assert int(from_all.sum()) == 2994  # (rows with hits from all three ranks)
    empty = np.flatnonzero(np.diff(indptr) == 0)
    assert empty.size == 4 and all(np.any((empty >= lo) & (empty < hi)) for lo, hi in blocks)
    for r in RADII:
        ip, ix, ds = merge_sparse_radius(_shard_parts(D, blocks, r))
        for e in empty:  # an empty row: the four empty rows at distance 0, in index order, from all three ranks
            assert ix[ip[e]:ip[e + 1]].tolist() == empty.tolist() and np.all(ds[ip[e]:ip[e + 1]] == 0)


def _csr(*rows_):
    ip = np.zeros(len(rows_) + 1, np.int64)
    np.cumsum([len(r) for r in rows_], out=ip[1:])
    flat = [e for r in rows_ for e in r]
    return (ip, np.array([e[0] for e in flat], np.int32).reshape(-1), np.array([e[1] for e in flat], np.float32).reshape(-1))


def test_small_cases_by_hand():
    a = _csr([(4, 0.0), (9, 0.25)], [], [(1, 0.5)])
    b = _csr([(2, 0.25)], [(7, 0.0)], [(0, 0.5), (3, 0.5)])
    ip, ix, ds = merge_sparse_radius([a, b])
    assert ip.tolist() == [0, 3, 4, 7] and ix.tolist() == [4, 2, 9, 7, 0, 1, 3]
    assert ds.tolist() == [0.0, 0.25, 0.25, 0.0, 0.5, 0.5, 0.5]
    none = _csr([], [], [])  # an all-empty part changes nothing, wherever it stands
    for parts in ([none, a, b], [a, none, b], [a, b, none]):
        rmodel.same(merge_sparse_radius(parts), (ip, ix, ds))
    rmodel.same(merge_sparse_radius([none, none]), none)
    rmodel.same(merge_sparse_radius([a]), a)
    # equal keys in two parts: both come out, the earlier part's first (told apart here by nothing: so by the counts)
    dup = merge_sparse_radius([_csr([(4, 0.25), (9, 0.25)]), _csr([(4, 0.25)])])
    assert dup[1].tolist() == [4, 4, 9]


def test_no_queries_and_bad_parts():
    z = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    got = merge_sparse_radius([z, z, z])
    rmodel.same(got, z)
    with pytest.raises(ValueError, match="at least one part"):
        merge_sparse_radius([])
    a = _csr([(1, 0.0)], [])
    with pytest.raises(ValueError, match="same nq"):
        merge_sparse_radius([a, _csr([(2, 0.0)])])
    with pytest.raises(ValueError):
        merge_sparse_radius([(np.array([0, 2, 1], np.int64), a[1], a[2])])


def test_offsets_of_the_radius_search_have_no_k_but_need_a_row_on_every_rank():
    assert sparse_radius_offsets([1024, 1024, 952]) == [(0, 1024), (1024, 2048), (2048, 3000)]
    assert sparse_radius_offsets([1, 1]) == [(0, 1), (1, 2)]  # (no k: a rank of one row answers)
    with pytest.raises(ValueError, match="rank 1 of 3 holds no rows.*at least one row") as e:
        sparse_radius_offsets([5, 0, 0])
    with pytest.raises(ValueError) as again:
        sparse_radius_offsets((5, 0, 0))
    assert str(e.value) == str(again.value)  # (a function of the counts alone: the same on every rank)
    with pytest.raises(ValueError):
        sparse_radius_offsets([])


# ---- the entry point -----------------------------------------------------------------------------------------------------
def test_entry_point_follows_the_abi_conventions():
    from fedrann_amd import build
    build.build_library()
    L = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fedrann_hip.h")).read()
    m = re.search(r"^int fdr_radius_merge\(fdr_ctx \*ctx([^;]*)\);", hdr, re.M)
    assert m
    assert "fdr_radius_merge" in _lib.SYMBOLS and hasattr(L, "fdr_radius_merge")
    fn = L.fdr_radius_merge
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 1 + m.group(1).count(",") == 9
    ip = np.zeros(1, np.int64)
    assert fn(None, 0, 1, ip.ctypes.data, None, None, ip.ctypes.data, None, None) == -1  # FDR_E_ARG
    assert b"null context" in L.fdr_last_error()


# ---- Context.radius_merge: the checks come before the library -----------------------------------------------------------
class _NoLibrary(_lib.Context):
    """A context whose library must never be reached."""

    def __init__(self):
        self._h = None

    @property
    def _L(self):
        raise AssertionError("the library was called")


def _part(counts):
    ip = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=ip[1:])
    return ip, np.zeros(int(ip[-1]), np.int32), np.zeros(int(ip[-1]), np.float32)


def test_good_arguments_are_summed():
    n_parts, nq, counts = _lib.check_radius_merge([_part([1, 0, 3]), _part([0, 0, 2])])
    assert (n_parts, nq) == (2, 3) and counts.tolist() == [1, 0, 5] and counts.dtype == np.int64
    assert _lib.check_radius_merge([_part([])] * 64)[:2] == (64, 0)


def test_bad_indptrs_raise_before_the_library_is_called():
    c = _NoLibrary()
    good = _part([2, 1])
    for bad in (np.array([1, 2, 3], np.int64), np.array([0, 2, 1], np.int64), np.array([0, -1, 3], np.int64)):
        with pytest.raises(ValueError, match="start at 0 and never decrease"):
            c.radius_merge([good, (bad, good[1], good[2])])
    with pytest.raises(ValueError, match="nq \\+ 1"):
        c.radius_merge([good, _part([3])])
    with pytest.raises(ValueError, match="entries its indptr states"):
        c.radius_merge([good, (good[0], good[1][:2].copy(), good[2])])
    with pytest.raises(TypeError, match="indptr"):
        c.radius_merge([(good[0].astype(np.int32), good[1], good[2])])
    with pytest.raises(TypeError, match="idx"):
        c.radius_merge([(good[0], good[1].astype(np.int64), good[2])])
    with pytest.raises(TypeError, match="dist"):
        c.radius_merge([(good[0], good[1], good[2].astype(np.float64))])
    with pytest.raises(ValueError, match="triple"):
        c.radius_merge([good[:2]])
    for cap in (0, 2 ** 31, 2.0, True):
        with pytest.raises(ValueError, match="max_entries"):
            c.radius_merge([good], max_entries=cap)
    with pytest.raises(ValueError, match="query 0 alone has 4 entries"):
        c.radius_merge([good, good], max_entries=3)


def test_two_to_the_31_entries_raise_before_the_library_is_called():
    half = (np.array([0, 2 ** 30], np.int64), np.zeros(1, np.int32), np.zeros(1, np.float32))  # (never looked at)
    with pytest.raises(ValueError, match="2\\^31"):
        _NoLibrary().radius_merge([half, half])


def test_more_than_64_parts_raise_before_the_library_is_called():
    with pytest.raises(ValueError, match="n_parts"):
        _NoLibrary().radius_merge([_part([1])] * 65)
    with pytest.raises(ValueError, match="n_parts"):
        _NoLibrary().radius_merge([])


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE = ["-o", "out", "--feature-matrix", "x.npz", "--kmer-counts", "c.npy"]
RADIUS = ["--no-projection", "--no-projection-radius", "0.5"]


def test_targets_radius_and_several_devices_pass_the_checks():
    args = cli.parse_command_line_arguments(BASE + RADIUS + ["--devices", "0,1,2", "--sparse-shard", "targets"])
    cli.check_radius(args, "--no-projection-radius", args.no_projection_radius, True)
    cli.check_radius(args, "--radius", args.radius, False)
    cli.check_sparse_shard(args)
    one = cli.parse_command_line_arguments(BASE + RADIUS)  # (one GPU: as before)
    cli.check_radius(one, "--no-projection-radius", one.no_projection_radius, True)


@pytest.mark.parametrize("extra,words", [
    (RADIUS + ["--devices", "0,0"], ("one GPU", "--devices", "--sparse-shard targets")),
    (RADIUS + ["--devices", "0,0", "--sparse-shard", "queries"], ("one GPU", "--devices", "--sparse-shard targets")),
    (["--radius", "0.5", "--devices", "0,1"], ("one GPU", "--devices")),
])
def test_the_three_refusals_keep_their_words_and_come_before_any_work(tmp_path, extra, words):
    out_dir = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        cli.main(["-o", str(out_dir)] + BASE[2:] + extra)
    assert all(w in str(e.value) for w in words), e.value
    assert not os.path.exists(out_dir)  # refused before the output directory is made
