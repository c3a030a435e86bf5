"""The sparse index without a GPU: the range and k checks of SparseIndex.search, the argument checks that
Context.sparse_index shares with Context.knn_sparse, the query blocks of sparse_knn_rank, and the four entry points in
the header, the bindings and the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fedrann_amd import _lib
from fedrann_amd.distributed import shard_rows, sparse_rank_blocks

NEW = ("fdr_sparse_index_build", "fdr_sparse_index_search", "fdr_sparse_index_info", "fdr_sparse_index_free")


def _csr():
    indptr = np.array([0, 2, 4, 4, 6], np.int64)
    indices = np.array([1, 7, 0, 3, 2, 9], np.int32)
    values = np.array([1.0, -2.0, 0.5, 0.0, 3.0, 1.0], np.float32)
    return indptr, indices, values


# ---- SparseIndex.search: range and k ----------------------------------------------------------------------------------
def test_search_range_and_k_are_normalised():
    assert _lib.check_sparse_search(10, 3) == (3, 0, 10)
    assert _lib.check_sparse_search(10, 10, 4, 4) == (10, 4, 4)  # an empty range, k = n
    assert _lib.check_sparse_search(10, 5, 9, 10) == (5, 9, 10)  # a range shorter than k
    assert _lib.check_sparse_search(300, np.int64(128), np.int32(0), None) == (128, 0, 300)


@pytest.mark.parametrize("n,k,lo,hi", [(10, 0, 0, 10), (10, 11, 0, 10), (300, 129, 0, 300), (10, -1, 0, 1),
                                       (10, 3, -1, 5), (10, 3, 6, 5), (10, 3, 0, 11), (10, 3, 11, 11)])
def test_search_rejects_a_bad_range_or_k(n, k, lo, hi):
    with pytest.raises(ValueError):
        _lib.check_sparse_search(n, k, lo, hi)


@pytest.mark.parametrize("k,lo,hi", [(2.0, 0, 4), (2, 0.5, 4), (2, 0, "4"), (True, 0, 4)])
def test_search_rejects_non_integers(k, lo, hi):
    with pytest.raises(ValueError):
        _lib.check_sparse_search(10, k, lo, hi)


class _NoLibrary:
    """A context stand-in whose library must never be reached."""
    _h = 1
    _sparse_gen = 1

    @property
    def _L(self):
        raise AssertionError("the library was called")


def test_search_raises_before_the_library_is_called():
    index = _lib.SparseIndex(_NoLibrary(), 10, "cosine", 1)
    for k, lo, hi in ((0, 0, 10), (11, 0, 10), (3, 5, 4), (3, 0, 11), (3, -2, 4)):
        with pytest.raises(ValueError):
            index.search(k, lo, hi)
    with pytest.raises(ValueError, match="out"):
        index.search(3, 0, 4, out=(np.empty((4, 3), np.int32), np.empty((5, 3), np.float32)))
    with pytest.raises(ValueError, match="out"):
        index.search(3, 0, 4, out=(np.empty((4, 3), np.int64), np.empty((4, 3), np.float32)))


def test_a_stale_or_closed_index_raises_before_the_library_is_called():
    c = _NoLibrary()
    index = _lib.SparseIndex(c, 10, "cosine", 1)
    c._sparse_gen = 2  # the context built another index
    with pytest.raises(_lib.FedrannHipError, match="another sparse index"):
        index.search(3)
    with pytest.raises(_lib.FedrannHipError, match="another sparse index"):
        index.info()
    index.close()  # (frees nothing: the context's index is not this one)
    with pytest.raises(_lib.FedrannHipError, match="closed"):
        index.search(3)


# ---- the split argument checks ----------------------------------------------------------------------------------------
def test_index_checks_are_the_search_checks_without_k():
    indptr, indices, values = _csr()
    assert _lib.check_sparse_csr(indptr, indices, values, 10) == (4, 10)
    assert _lib.check_sparse_csr(indptr, indices, None, 10) == (4, 10)
    assert _lib.check_sparse_rows(indptr, indices, values, 10, 4) == (4, 4, 10)
    one = np.array([0, 0], np.int64)  # one empty row: an index (n >= 1), and a search at k = 1
    assert _lib.check_sparse_csr(one, np.zeros(0, np.int32), None, 1) == (1, 1)
    with pytest.raises(ValueError, match="row"):
        _lib.check_sparse_csr(np.array([0], np.int64), np.zeros(0, np.int32), None, 1)


def test_index_checks_reject_what_the_search_checks_reject():
    indptr, indices, values = _csr()
    cases = [
        (ValueError, "strictly ascending", (indptr, np.array([7, 1, 0, 3, 2, 9], np.int32), values, 10)),
        (ValueError, "strictly ascending", (indptr, np.array([1, 1, 0, 3, 2, 9], np.int32), values, 10)),
        (ValueError, "outside", (indptr, indices, values, 9)),
        (ValueError, "n_features", (indptr, indices, values, 0)),
        (ValueError, "indptr", (np.array([0, 2, 1, 4, 6], np.int64), indices, values, 10)),
        (ValueError, "differ in length", (indptr, indices, values[:5].copy(), 10)),
        (TypeError, "indptr", (indptr.astype(np.int32), indices, values, 10)),
        (TypeError, "values", (indptr, indices, values.astype(np.float64), 10)),
    ]
    bad = values.copy()
    bad[3] = np.nan
    cases.append((ValueError, "finite", (indptr, indices, bad, 10)))
    for exc, match, args in cases:
        with pytest.raises(exc, match=match) as e_index:
            _lib.check_sparse_csr(*args)
        with pytest.raises(exc, match=match) as e_rows:
            _lib.check_sparse_rows(*args, 2)
        assert str(e_index.value) == str(e_rows.value)  # one implementation: the same words


# ---- sparse_knn_rank's blocks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 64, 1001])
@pytest.mark.parametrize("world", [1, 2, 3, 7])
@pytest.mark.parametrize("block_rows", [None, 1, 7, 700])
def test_rank_blocks_tile_the_rows(n, world, block_rows):
    at = 0
    for rank in range(world):
        lo, hi, blocks = sparse_rank_blocks(n, rank, world, block_rows)
        assert (lo, hi) == shard_rows(n, world)[1][rank] and lo == at
        for a, b in blocks:
            assert a == at and a < b <= hi and (block_rows is None or b - a <= block_rows)
            at = b
        assert at == hi
        if block_rows is None:
            assert len(blocks) == (1 if hi > lo else 0)
    assert at == n


def test_rank_blocks_reject_bad_arguments():
    for rank, world, block_rows in ((2, 2, None), (-1, 2, None), (0, 0, None), (0, 2, 0)):
        with pytest.raises(ValueError):
            sparse_rank_blocks(10, rank, world, block_rows)


# ---- the entry points -------------------------------------------------------------------------------------------------
def test_new_entry_points_follow_the_abi_conventions():
    """Declared in the header as int functions of (fdr_ctx *ctx, ...), listed in _lib.SYMBOLS, exported by the
    library, bound with an int return and one argument type per parameter."""
    from fedrann_amd import build
    build.build_library()
    L = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fedrann_hip.h")).read()
    for name in NEW:
        m = re.search(r"^int %s\(fdr_ctx \*ctx([^;]*)\);" % name, hdr, re.M)
        assert m, name
        n_params = 1 + m.group(1).count(",")
        assert name in _lib.SYMBOLS and hasattr(L, name)
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_params, name


def test_new_entry_points_refuse_a_null_context():
    L = _lib.load_library()
    assert L.fdr_sparse_index_build(None, 0, 1, 1, None, None, None) == -1  # FDR_E_ARG
    assert L.fdr_sparse_index_search(None, 1, 0, 0, None, None) == -1
    assert L.fdr_sparse_index_info(None, None, None, None, None, None) == -1
    assert L.fdr_sparse_index_free(None) == -1
