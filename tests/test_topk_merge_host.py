"""fdr_topk_merge and the target-sharded sparse search without a GPU: the entry point in the header, the bindings and
the library; the argument checks of Context.topk_merge, which raise before the library is called; the k check of
sparse_knn_sharded; --sparse-shard on the command line."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fedrann_amd import __main__ as cli
from fedrann_amd import _lib
from fedrann_amd.distributed import shard_rows, sparse_shard_offsets


# ---- the entry point ----------------------------------------------------------------------------------------------------
def test_entry_point_follows_the_abi_conventions():
    from fedrann_amd import build
    build.build_library()
    L = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fedrann_hip.h")).read()
    m = re.search(r"^int fdr_topk_merge\(fdr_ctx \*ctx([^;]*)\);", hdr, re.M)
    assert m
    assert "fdr_topk_merge" in _lib.SYMBOLS and hasattr(L, "fdr_topk_merge")
    fn = L.fdr_topk_merge
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 1 + m.group(1).count(",") == 9


def test_entry_point_refuses_a_null_context():
    from fedrann_amd import build
    build.build_library()
    L = _lib.load_library()
    assert L.fdr_topk_merge(None, 0, 1, 1, 1, None, None, None, None) == -1  # FDR_E_ARG
    assert b"null context" in L.fdr_last_error()
    idx, dist = np.zeros((2, 3, 4), np.int32), np.zeros((2, 3, 4), np.float32)
    out = np.zeros((3, 4), np.int32), np.zeros((3, 4), np.float32)
    assert L.fdr_topk_merge(None, 3, 2, 4, 4, idx.ctypes.data, dist.ctypes.data, out[0].ctypes.data,
                            out[1].ctypes.data) == -1


# ---- Context.topk_merge: the checks come before the library -------------------------------------------------------------
class _NoLibrary(_lib.Context):
    """A context whose library must never be reached."""

    def __init__(self):
        self._h = None

    @property
    def _L(self):
        raise AssertionError("the library was called")


def _parts(n_parts, nq, kp):
    return np.zeros((n_parts, nq, kp), np.int32), np.zeros((n_parts, nq, kp), np.float32)


def test_good_arguments_are_normalised():
    assert _lib.check_topk_merge(*_parts(3, 5, 20), 20) == (3, 5, 20, 20)
    assert _lib.check_topk_merge(*_parts(64, 0, 1), np.int64(64)) == (64, 0, 1, 64)
    assert _lib.check_topk_merge(*_parts(2, 7, 128), 128) == (2, 7, 128, 128)
    out = np.empty((5, 9), np.int32), np.empty((5, 9), np.float32)
    assert _lib.check_topk_merge(*_parts(3, 5, 4), 9, out) == (3, 5, 4, 9)


@pytest.mark.parametrize("shape,k,match", [
    ((0, 5, 20), 1, "n_parts"), ((65, 5, 20), 20, "n_parts"),
    ((2, 5, 20), 0, "k"), ((2, 5, 128), 129, "k"), ((2, 5, 20), -1, "k"),
    ((2, 5, 20), 41, "n_parts \\* kp"), ((1, 5, 1), 2, "n_parts \\* kp"),
    ((2, 5, 0), 1, "kp"), ((2, 5, 129), 1, "kp"),
])
def test_limits_raise_before_the_library_is_called(shape, k, match):
    with pytest.raises(ValueError, match=match):
        _NoLibrary().topk_merge(*_parts(*shape), k)


def test_shapes_and_dtypes_raise_before_the_library_is_called():
    c = _NoLibrary()
    idx, dist = _parts(2, 5, 20)
    with pytest.raises(ValueError, match="differ in shape"):
        c.topk_merge(idx, dist[:, :4].copy(), 20)
    with pytest.raises(ValueError, match="differ in shape"):
        c.topk_merge(idx, np.zeros((2, 20, 5), np.float32), 20)
    with pytest.raises(ValueError, match="n_parts, nq, kp"):
        c.topk_merge(idx[0], dist[0], 20)  # one part's [nq, kp] alone
    with pytest.raises(ValueError, match="C-contiguous"):
        c.topk_merge(np.zeros((5, 2, 20), np.int32).transpose(1, 0, 2), dist, 20)  # query-major: not the layout
    with pytest.raises(TypeError, match="idx_parts"):
        c.topk_merge(idx.astype(np.int64), dist, 20)
    with pytest.raises(TypeError, match="dist_parts"):
        c.topk_merge(idx, dist.astype(np.float64), 20)
    with pytest.raises(TypeError, match="idx_parts"):
        c.topk_merge(idx.tolist(), dist, 20)
    for k in (2.0, True, "3"):
        with pytest.raises(ValueError, match="integer"):
            c.topk_merge(idx, dist, k)
    with pytest.raises(ValueError, match="out"):
        c.topk_merge(idx, dist, 20, out=(np.empty((5, 20), np.int32), np.empty((5, 19), np.float32)))
    with pytest.raises(ValueError, match="out"):
        c.topk_merge(idx, dist, 20, out=(np.empty((5, 20), np.int64), np.empty((5, 20), np.float32)))


# ---- the k check of the target-sharded search ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1001, 3000])
@pytest.mark.parametrize("world", [1, 2, 3, 7])
def test_offsets_tile_shard_rows(n, world):
    blocks = shard_rows(n, world)[1]
    counts = [hi - lo for lo, hi in blocks]
    k = min(counts)
    if k == 0:
        with pytest.raises(ValueError, match="holds 0 target rows"):
            sparse_shard_offsets(counts, 1)
        return
    assert sparse_shard_offsets(counts, k) == blocks
    assert sparse_shard_offsets(counts, 1) == blocks


def test_offsets_name_the_short_rank():
    counts = [hi - lo for lo, hi in shard_rows(3000, 3)[1]]
    assert counts == [1024, 1024, 952]
    assert sparse_shard_offsets(counts, 952)[2] == (2048, 3000)
    with pytest.raises(ValueError, match=r"rank 2 of 3 holds 952 target rows.*k = 953") as e:
        sparse_shard_offsets(counts, 953)
    with pytest.raises(ValueError) as again:
        sparse_shard_offsets(list(counts), 953)
    assert str(e.value) == str(again.value)  # (a function of the counts and k alone: the same on every rank)
    with pytest.raises(ValueError, match="rank 1 of 4 holds 3 "):
        sparse_shard_offsets([10, 3, 7, 3], 4)  # the first of the shortest
    assert sparse_shard_offsets([10, 3, 7, 3], 3) == [(0, 10), (10, 13), (13, 20), (20, 23)]
    with pytest.raises(ValueError):
        sparse_shard_offsets([], 1)


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE = ["-o", "out", "--feature-matrix", "x.npz", "--kmer-counts", "c.npy"]


@pytest.mark.parametrize("mode", ["targets", "queries"])
def test_parser_accepts_sparse_shard(mode):
    args = cli.parse_command_line_arguments(BASE + ["--no-projection", "--devices", "0,1", "--sparse-shard", mode])
    assert args.sparse_shard == mode
    cli.check_sparse_shard(args)  # (nothing to refuse)
    assert cli.parse_command_line_arguments(BASE).sparse_shard is None
    cli.check_sparse_shard(cli.parse_command_line_arguments(BASE + ["--no-projection"]))
    cli.check_sparse_shard(cli.parse_command_line_arguments(BASE + ["--devices", "0,1"]))


def test_parser_rejects_another_value(capsys):
    with pytest.raises(SystemExit):
        cli.parse_command_line_arguments(BASE + ["--no-projection", "--devices", "0,1", "--sparse-shard", "rows"])
    assert "--sparse-shard" in capsys.readouterr().err


@pytest.mark.parametrize("extra,needs", [
    (["--devices", "0,1", "--sparse-shard", "targets"], "--no-projection"),
    (["--no-projection", "--sparse-shard", "queries"], "--devices"),
    (["--no-projection", "--devices", "3", "--sparse-shard", "targets"], "--devices"),
    (["--no-projection", "--devices", "0,", "--sparse-shard", "targets"], "--devices"),
])
def test_sparse_shard_is_refused_without_what_it_needs(extra, needs, tmp_path):
    args = cli.parse_command_line_arguments(BASE + extra)
    with pytest.raises(SystemExit) as e:
        cli.check_sparse_shard(args)
    assert "--sparse-shard" in str(e.value) and needs in str(e.value)
    with pytest.raises(SystemExit) as e:  # main() refuses before it makes the output directory
        cli.main(["-o", str(tmp_path / "out")] + BASE[2:] + extra)
    assert needs in str(e.value) and not (tmp_path / "out").exists()


def test_several_devices_without_the_flag_name_it(tmp_path):
    args = cli.parse_command_line_arguments(BASE + ["--no-projection", "--devices", "0,1"])
    with pytest.raises(SystemExit) as e:
        cli.check_sparse_shard(args)
    msg = str(e.value)
    assert "--no-projection" in msg and "--devices" in msg and msg.endswith("--sparse-shard targets|queries")
