"""Exact Jaccard k-NN on sparse feature rows (fdr_knn_sparse_metric, FDR_METRIC_JACCARD): indices and distance bits
against the numpy / scipy model of tests/_jaccard_model.py, stored zeros as absent entries, tie plateaus, long
queries, the range-split path, cosine through the new entry point, argument errors, NNDescent_ava(metric="jaccard")
and the --no-projection-metric command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import _jaccard_model as model
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([r[0].size for r in rows])
    indices = np.concatenate([r[0] for r in rows]).astype(np.int32)
    values = np.concatenate([r[1] for r in rows]).astype(np.float32)
    return indptr, indices, values


def _set_rows(n, seed, F=1 << 25, n_ids=512, per=(1, 12), zeros=0.1):
    """CSR rows over feature ids spread across [0, F) but drawn from n_ids distinct ids: about 10 % explicit stored
    zeros, empty rows, rows of stored zeros only, exact duplicates, rows with equal sets under different values, and
    isolated rows (ids no other row holds).  Returns (indptr, indices, values)."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(F, n_ids, replace=False)).astype(np.int64)
    n_iso = min(64, n_ids // 4)
    iso = pool[-n_iso:]  # the isolated rows' private ids
    rows = []
    for i in range(n):
        m = int(rng.integers(per[0], per[1] + 1))
        ids = np.sort(rng.choice(pool[:-n_iso], m, replace=False))
        vals = (rng.integers(1, 6, size=m) * 0.37 * rng.choice([-1.0, 1.0], size=m)).astype(np.float32)
        vals[rng.random(m) < zeros] = 0.0  # explicit stored zeros: absent from the set
        rows.append((ids, vals))
    for i in range(0, n, 97):
        rows[i] = (np.zeros(0, np.int64), np.zeros(0, np.float32))  # empty row
    for i in range(5, n, 131):
        ids = rows[i][0]
        rows[i] = (ids, np.where(np.arange(ids.size) % 2 == 0, 0.0, -0.0).astype(np.float32))  # only +-0: an empty set
    if n > 4:
        for i in range(7, n, 53):
            rows[i] = rows[3]  # duplicates
        for i in range(11, n, 71):
            ids, vals = rows[4]
            rows[i] = (ids, np.where(vals != 0, np.float32(-9.5), np.float32(0)).astype(np.float32))  # equal sets
    for j, i in enumerate(range(13, n, max(1, n // 64))):
        if j < iso.size:
            rows[i] = (iso[j:j + 1], np.array([1.5], np.float32))  # isolated: alone with its id
    return _csr(rows)


def _same(a, b):
    ai, ad = a
    bi, bd = b
    assert ai.shape == bi.shape
    bad = np.flatnonzero(np.any((ai != bi) | (ad.view(np.uint32) != bd.view(np.uint32)), axis=1))
    assert bad.size == 0, "rows differ: %s (first: got %s %s, want %s %s)" % (
        bad[:10], ai[bad[0]], ad[bad[0]], bi[bad[0]], bd[bad[0]])


def _same_rows(got, rows, want):
    _same((got[0][rows], got[1][rows]), want)


# ---- 1. every row against the model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hard():
    rows = _set_rows(4000, seed=1701)
    want = model.knn_all(*rows, 1 << 25, 128)  # (a prefix of the (dist, index) order is the smaller k's answer)
    return rows, want


@pytest.mark.parametrize("k", [1, 20, 64, 128])
def test_every_row_matches_the_model(ctx, hard, k):
    (indptr, indices, values), (wi, wd) = hard
    got = ctx.knn_sparse(indptr, indices, values, 1 << 25, k, metric="jaccard")
    assert ctx.last_knn_trace()["kind"] == "sparse"
    _same(got, (wi[:, :k], wd[:, :k]))


def test_trace_counts_the_empty_rows(ctx, hard):
    (indptr, indices, values), _ = hard
    ctx.knn_sparse(indptr, indices, values, 1 << 25, 20, metric="jaccard")
    sizes = model.binary_csr(indptr, indices, values, 1 << 25).getnnz(1)
    t = ctx.last_knn_trace()
    assert t["zero_queries"] == int(np.sum(sizes == 0)) > 0 and t["queries"] == t["targets"] == 4000 and t["k"] == 20


# ---- 2. values=None against values given ----------------------------------------------------------------------------
def test_a_stored_zero_is_absent(ctx):
    F, k = 1 << 25, 20
    indptr, indices, values = _set_rows(3000, seed=9, n_ids=300, zeros=0.0)
    nz = np.where(values == 0, np.float32(1.25), values)  # (the rows of stored zeros only become plain rows)
    assert np.all(nz != 0)
    all_present = ctx.knn_sparse(indptr, indices, None, F, k, metric="jaccard")
    _same(ctx.knn_sparse(indptr, indices, nz, F, k, metric="jaccard"), all_present)
    _same(all_present, model.knn_all(indptr, indices, None, F, k))
    some = nz.copy()
    some[np.random.default_rng(10).random(some.size) < 0.25] = 0.0
    smaller = ctx.knn_sparse(indptr, indices, some, F, k, metric="jaccard")
    _same(smaller, model.knn_all(indptr, indices, some, F, k))
    assert np.any(smaller[0] != all_present[0])


# ---- 3. n == k --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 128])
def test_n_equals_k(ctx, n):
    indptr, indices, values = _set_rows(n, seed=n, F=1 << 24, n_ids=128, per=(1, 4))
    _same(ctx.knn_sparse(indptr, indices, values, 1 << 24, n, metric="jaccard"),
          model.knn_all(indptr, indices, values, 1 << 24, n))


# ---- 4. tie plateaus --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plateaus():
    """3000 rows, each a subset of 8 ids (the empty subset included): every distance is c / u with u <= 8, and equal
    ratios come from different (c, u), such as 1/2 and 2/4."""
    rng = np.random.default_rng(8)
    ids = np.sort(rng.choice(1 << 20, 8, replace=False)).astype(np.int64)
    masks = rng.integers(0, 256, size=3000)
    rows = [ids[((m >> np.arange(8)) & 1) == 1] for m in masks]
    rows = [(r, np.ones(r.size, np.float32)) for r in rows]
    csr = _csr(rows)
    return csr, model.knn_all(*csr, 1 << 20, 128)


@pytest.mark.parametrize("k", [20, 128])
def test_tie_plateaus_keep_the_index_order(ctx, plateaus, k):
    (indptr, indices, values), (wi, wd) = plateaus
    assert np.unique(wd).size <= 23 and np.any(wd == np.float32(0.5))  # (the Farey fractions up to 1/8 steps)
    got = ctx.knn_sparse(indptr, indices, values, 1 << 20, k, metric="jaccard")
    _same(got, (wi[:, :k], wd[:, :k]))


# ---- 5. long queries --------------------------------------------------------------------------------------------------
def test_long_queries(ctx):
    """1-300 entries from 2000 ids: the query walk takes several 64-entry rounds.  Every fourth row is short (its
    table comes close to SP_LIMIT = 512 targets, on either side), every fourth is long over 6000 ids of its own kind
    (several rounds into one table of at most 375 targets); the rest pass SP_LIMIT and take the range split."""
    rng = np.random.default_rng(15)
    n, F = 1500, 8000
    rows = []
    for i in range(n):
        if i % 4 == 1:
            ids = 2000 + np.sort(rng.choice(6000, int(rng.integers(70, 251)), replace=False)).astype(np.int64)
        else:
            m = int(rng.integers(1, 301)) if i % 4 else int(rng.integers(1, 6))
            ids = np.sort(rng.choice(2000, m, replace=False)).astype(np.int64)
        m = ids.size
        vals = np.ones(m, np.float32)
        vals[rng.random(m) < 0.05] = 0.0
        rows.append((ids, vals))
    indptr, indices, values = _csr(rows)
    got = ctx.knn_sparse(indptr, indices, values, F, 20, metric="jaccard")
    _same(got, model.knn_all(indptr, indices, values, F, 20))


# ---- 6. range split ---------------------------------------------------------------------------------------------------
def _heavy_rows(n, seed):
    """Feature 0 in every row, a few medium features (df ~ n / 50) and private-ish light ones."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        ids = {0, 1 + int(rng.integers(0, 50)), 100 + int(rng.integers(0, 5000))}
        if i % 3 == 0:
            ids.add(6000 + int(rng.integers(0, 100000)))
        ids = np.array(sorted(ids), np.int64)
        vals = (rng.integers(1, 8, size=ids.size) * 0.25).astype(np.float32)
        if i % 11 == 0:
            vals[-1] = 0.0  # (feature 0 stays present in every row)
        rows.append((ids, vals))
    return _csr(rows)


def test_heavy_postings_take_the_range_split(ctx):
    n, F, k = 20000, 1 << 24, 20
    indptr, indices, values = _heavy_rows(n, seed=5)
    got = ctx.knn_sparse(indptr, indices, values, F, k, metric="jaccard")
    t = ctx.last_knn_trace()
    assert t["kind"] == "sparse" and t["range_queries"] > 0 and t["range_chunks"] > 1, t
    rng = np.random.default_rng(3)
    rows = np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), rng.choice(n, 40, replace=False)]))
    _same_rows(got, rows, model.knn_rows(indptr, indices, values, F, k, rows))


# ---- 7. cosine through the new entry point ----------------------------------------------------------------------------
def _raw_call(ctx, metric, indptr, indices, values, F, k):
    n = indptr.size - 1
    idx = np.empty((n, k), np.int32)
    dist = np.empty((n, k), np.float32)
    vp = ctypes.c_void_p
    rc = ctx._L.fdr_knn_sparse_metric(ctx._h, metric, n, F, vp(indptr.ctypes.data), vp(indices.ctypes.data),
                                      vp(values.ctypes.data) if values is not None else None, k,
                                      vp(idx.ctypes.data), vp(dist.ctypes.data))
    return rc, idx, dist


def test_cosine_through_the_metric_entry_point(ctx):
    indptr, indices, values = _set_rows(3000, seed=31)
    want = ctx.knn_sparse(indptr, indices, values, 1 << 25, 20)
    rc, idx, dist = _raw_call(ctx, _lib.METRIC_COSINE, indptr, indices, values, 1 << 25, 20)
    assert rc == 0 and ctx.last_knn_trace()["kind"] == "sparse"
    _same((idx, dist), want)
    _same(ctx.knn_sparse(indptr, indices, values, 1 << 25, 20, metric="cosine"), want)


# ---- 8. arguments -----------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    F = 1 << 20
    indptr, indices, values = _set_rows(200, seed=2, F=F, n_ids=128)
    E_ARG = -1
    j = int(indptr[20])  # row 20 holds at least one entry (not one of the emptied rows)
    assert indptr[21] > j
    bad = values.copy()
    bad[j] = np.nan
    with pytest.raises((ValueError, _lib.FedrannHipError)):
        ctx.knn_sparse(indptr, indices, bad, F, 5, metric="jaccard")
    assert _raw_call(ctx, _lib.METRIC_JACCARD, indptr, indices, bad, F, 5)[0] == E_ARG
    bad[j] = np.inf
    assert _raw_call(ctx, _lib.METRIC_JACCARD, indptr, indices, bad, F, 5)[0] == E_ARG
    two = np.flatnonzero(np.diff(indptr) >= 2)[0]
    desc = indices.copy()
    a = int(indptr[two])
    desc[a], desc[a + 1] = indices[a + 1], indices[a]
    with pytest.raises((ValueError, _lib.FedrannHipError)):
        ctx.knn_sparse(indptr, desc, values, F, 5, metric="jaccard")
    assert _raw_call(ctx, _lib.METRIC_JACCARD, indptr, desc, values, F, 5)[0] == E_ARG
    big = indices.copy()
    big[indptr[two + 1] - 1] = F
    with pytest.raises((ValueError, _lib.FedrannHipError)):
        ctx.knn_sparse(indptr, big, values, F, 5, metric="jaccard")
    assert _raw_call(ctx, _lib.METRIC_JACCARD, indptr, big, values, F, 5)[0] == E_ARG
    with pytest.raises((ValueError, _lib.FedrannHipError)):
        ctx.knn_sparse(indptr[:4], indices[:indptr[3]], values[:indptr[3]], F, 5, metric="jaccard")  # k > n
    assert _raw_call(ctx, _lib.METRIC_JACCARD, indptr[:4].copy(), indices, values, F, 5)[0] == E_ARG
    for metric in (2, -1, 7):
        assert _raw_call(ctx, metric, indptr, indices, values, F, 5)[0] == E_ARG
        assert b"metric" in ctx._L.fdr_last_error()
    got = ctx.knn_sparse(indptr, indices, values, F, 5, metric="jaccard")  # (the context is fine afterwards)
    _same(got, model.knn_all(indptr, indices, values, F, 5))


# ---- 9. NNDescent_ava(metric="jaccard") -----------------------------------------------------------------------------
def test_nndescent_jaccard_sparse_and_dense_input(ctx):
    from fedrann_amd.nearest_neighbors import NNDescent_ava
    indptr, indices, values = _set_rows(2000, seed=22, F=1024, n_ids=1024)
    A = sp.csr_matrix((values, indices, indptr), shape=(2000, 1024))
    want = model.knn_all(indptr, indices, values, 1024, 20)
    got = NNDescent_ava().get_neighbors(A, metric="jaccard", index_n_neighbors=20, context=ctx, verbose=False)
    assert ctx.last_knn_trace()["kind"] == "sparse"
    _same(got, want)
    got = NNDescent_ava().get_neighbors(A.toarray(), metric="jaccard", index_n_neighbors=20, context=ctx,
                                        verbose=False)
    assert ctx.last_knn_trace()["kind"] == "sparse"
    _same(got, want)
    with pytest.raises(ValueError, match="cosine.*jaccard"):
        NNDescent_ava().get_neighbors(A, metric="euclidean", index_n_neighbors=20, context=ctx, verbose=False)


# ---- 10. the command line -------------------------------------------------------------------------------------------
def test_cli_no_projection_metric_jaccard(ctx, tmp_path):
    from fedrann_amd.__main__ import write_overlaps
    from fedrann_amd.feature_extraction import save_feature_matrix_npz
    from fedrann_amd.synth import synth
    s = synth(3000, seed=44, doubling=True)
    fm, cnt = str(tmp_path / "feature_matrix.npz"), str(tmp_path / "counts.npy")
    save_feature_matrix_npz(fm, s["indptr"], s["indices"], s["n_features"])
    np.save(cnt, s["counts"])
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "fedrann_amd", "-o", str(out), "--feature-matrix", fm, "--kmer-counts",
                        cnt, "--no-projection", "--no-projection-metric", "jaccard", "--nndescent-n-neighbors", "20"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "jaccard" in r.stderr and "values=None" in r.stderr  # (the log: stage 4's metric, stage 2 without weights)
    idx, dist = ctx.knn_sparse(s["indptr"], s["indices"], None, s["n_features"], 20, metric="jaccard")
    want = tmp_path / "want.tsv"
    n = s["indptr"].size - 1
    write_overlaps(str(want), idx, dist, ["row_%d" % i for i in range(n)], [0] * n)  # (no --read-names)
    assert (out / "overlaps.tsv").read_bytes() == want.read_bytes()
    rows = np.random.default_rng(12).choice(n, 100, replace=False)
    _same_rows((idx, dist), rows, model.knn_rows(s["indptr"], s["indices"], None, s["n_features"], 20, rows))
