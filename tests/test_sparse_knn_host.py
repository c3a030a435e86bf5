"""Sparse k-NN without a GPU: the argument checks of Context.knn_sparse, and the oracle-only fact the GPU tests of
fdr_knn_sparse rest on -- dropping the columns no row uses (keeping the others in ascending order) changes no k-NN
result, because every chain keeps its non-zero terms in the same order."""
import numpy as np
import pytest

from fedrann_amd import _lib


def _csr():
    indptr = np.array([0, 2, 4, 4, 6], np.int64)
    indices = np.array([1, 7, 0, 3, 2, 9], np.int32)
    values = np.array([1.0, -2.0, 0.5, 0.0, 3.0, 1.0], np.float32)
    return indptr, indices, values


def test_accepts_a_canonical_csr():
    indptr, indices, values = _csr()
    assert _lib.check_sparse_rows(indptr, indices, values, 10, 4) == (4, 4, 10)
    assert _lib.check_sparse_rows(indptr, indices, None, 10, 1) == (4, 1, 10)


@pytest.mark.parametrize("bad", [[7, 1, 0, 3, 2, 9], [1, 1, 0, 3, 2, 9]], ids=["unsorted", "duplicate"])
def test_rejects_unsorted_or_duplicate_indices(bad):
    indptr, _, values = _csr()
    with pytest.raises(ValueError, match="strictly ascending"):
        _lib.check_sparse_rows(indptr, np.array(bad, np.int32), values, 10, 2)


@pytest.mark.parametrize("v", [np.inf, -np.inf, np.nan])
def test_rejects_non_finite_values(v):
    indptr, indices, values = _csr()
    values[3] = v
    with pytest.raises(ValueError, match="finite"):
        _lib.check_sparse_rows(indptr, indices, values, 10, 2)


def test_rejects_k_above_n_and_bad_shapes():
    indptr, indices, values = _csr()
    with pytest.raises(ValueError, match="k"):
        _lib.check_sparse_rows(indptr, indices, values, 10, 5)
    with pytest.raises(ValueError, match="k"):
        _lib.check_sparse_rows(indptr, indices, values, 10, 0)
    with pytest.raises(ValueError, match="outside"):
        _lib.check_sparse_rows(indptr, indices, values, 9, 2)
    with pytest.raises(TypeError):
        _lib.check_sparse_rows(indptr.astype(np.int32), indices, values, 10, 2)
    with pytest.raises(TypeError):
        _lib.check_sparse_rows(indptr, indices, values.astype(np.float64), 10, 2)
    with pytest.raises(ValueError, match="indptr"):
        _lib.check_sparse_rows(np.array([0, 2, 1, 4, 6], np.int64), indices, values, 10, 2)


def test_column_compaction_keeps_every_knn_result(oracle):
    rng = np.random.default_rng(4)
    n, F, k = 600, 3000, 20
    D = np.zeros((n, F), np.float32)
    cols = rng.choice(F, 90, replace=False)  # the columns any row uses
    for i in range(n):
        c = rng.choice(cols, int(rng.integers(1, 8)), replace=False)
        D[i, c] = (rng.integers(-4, 5, size=c.size) * 0.41).astype(np.float32)  # (some stored zeros)
    D[::37] = 0.0
    D[5::29] = D[2]
    D[6::31] = 3.0 * D[1]
    used = np.flatnonzero(np.any(D != 0, axis=0))
    wi, wd = oracle.knn(D, k)
    gi, gd = oracle.knn(np.ascontiguousarray(D[:, used]), k)
    assert np.array_equal(wi, gi)
    assert np.array_equal(wd.view(np.uint32), gd.view(np.uint32))
    _, r_full, z_full = oracle.normalize(D)
    _, r_comp, z_comp = oracle.normalize(np.ascontiguousarray(D[:, used]))
    assert np.array_equal(r_full.view(np.uint32), r_comp.view(np.uint32)) and np.array_equal(z_full, z_comp)
