"""Exact cosine k-NN on sparse feature rows (fdr_knn_sparse): indices and distance bits against the oracle on the
densified rows, identity with the dense route, the range-split path under heavy postings, synthetic reads at scale,
NNDescent_ava on a csr_matrix wider than FDR_MAX_DIM, and the --no-projection command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hard_rows(n, seed, F=1 << 25, n_ids=512, per=(1, 12)):
    """CSR rows over feature ids spread across [0, F) but drawn from n_ids distinct ids: negative values, explicit
    stored zeros, empty rows, rows of explicit zeros only, exact duplicates, scaled copies, and isolated rows (ids
    no other row holds).  Returns (indptr, indices, values, pool) with pool = the distinct ids, ascending."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(F, n_ids, replace=False)).astype(np.int64)
    iso = pool[-64:]  # the isolated rows' private ids
    rows = []
    for i in range(n):
        m = int(rng.integers(per[0], per[1] + 1))
        ids = np.sort(rng.choice(pool[:-64], m, replace=False))
        vals = (rng.integers(1, 6, size=m) * 0.37 * rng.choice([-1.0, 1.0], size=m)).astype(np.float32)
        vals[rng.random(m) < 0.1] = 0.0  # explicit stored zeros
        rows.append((ids, vals))
    for i in range(0, n, 97):
        rows[i] = (np.zeros(0, np.int64), np.zeros(0, np.float32))  # empty row
    for i in range(5, n, 131):
        ids = rows[i][0]
        rows[i] = (ids, np.zeros(ids.size, np.float32))  # only explicit zeros: a zero row
    for i in range(7, n, 53):
        rows[i] = rows[3]  # duplicates
    for i in range(11, n, 71):
        rows[i] = (rows[4][0], (np.float32(2.5) * rows[4][1]).astype(np.float32))  # scaled copies
    for j, i in enumerate(range(13, n, max(1, n // 64))):
        if j < iso.size:
            rows[i] = (iso[j:j + 1], np.array([1.5], np.float32))  # isolated: alone with its id
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([r[0].size for r in rows])
    indices = np.concatenate([r[0] for r in rows]).astype(np.int32)
    values = np.concatenate([r[1] for r in rows]).astype(np.float32)
    return indptr, indices, values, pool


def _compact_dense(indptr, indices, values, pool):
    """The rows densified over the distinct ids in ascending order (every chain keeps its order and terms)."""
    n = indptr.size - 1
    D = np.zeros((n, pool.size), np.float32)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    D[rows, np.searchsorted(pool, indices)] = values
    return D


def _oracle_all(oracle, D, k):
    Eh, _, zero = oracle.normalize(D)
    return oracle.knn_normalized(Eh, zero, Eh, zero, k)


def _same(a, b):
    ai, ad = a
    bi, bd = b
    assert ai.shape == bi.shape
    bad = np.flatnonzero(np.any((ai != bi) | (ad.view(np.uint32) != bd.view(np.uint32)), axis=1))
    assert bad.size == 0, "rows differ: %s (first: got %s %s, want %s %s)" % (
        bad[:10], ai[bad[0]], ad[bad[0]], bi[bad[0]], bd[bad[0]])


@pytest.fixture(scope="module")
def hard():
    return _hard_rows(20000, seed=1701)


@pytest.mark.parametrize("k", [1, 20, 50, 64, 128])
def test_every_row_matches_the_oracle(ctx, oracle, hard, k):
    indptr, indices, values, pool = hard
    got = ctx.knn_sparse(indptr, indices, values, 1 << 25, k)
    assert ctx.last_knn_trace()["kind"] == "sparse"
    _same(got, _oracle_all(oracle, _compact_dense(indptr, indices, values, pool), k))


def test_ones_when_values_are_absent(ctx, oracle):
    indptr, indices, _, pool = _hard_rows(3000, seed=9, n_ids=300)
    got = ctx.knn_sparse(indptr, indices, None, 1 << 25, 20)
    _same(got, _oracle_all(oracle, _compact_dense(indptr, indices, np.ones(indices.size, np.float32), pool), 20))


@pytest.mark.parametrize("n", [1, 5, 64, 128])
def test_n_equals_k(ctx, oracle, n):
    indptr, indices, values, pool = _hard_rows(n, seed=n, F=1 << 24, n_ids=128, per=(1, 4))
    _same(ctx.knn_sparse(indptr, indices, values, 1 << 24, n),
          _oracle_all(oracle, _compact_dense(indptr, indices, values, pool), n))


@pytest.mark.parametrize("k", [20, 128])
def test_identical_to_the_dense_route(ctx, k):
    """At <= FDR_MAX_DIM columns the densified rows go through fdr_knn: the same bits."""
    indptr, indices, values, _ = _hard_rows(12000, seed=77, F=2048, n_ids=2048, per=(1, 16))
    A = sp.csr_matrix((values, indices, indptr), shape=(12000, 2048))
    _same(ctx.knn_sparse(indptr, indices, values, 2048, k), ctx.knn(A.toarray(), k))


# ---- per-query model for large inputs -------------------------------------------------------------------------------
def _row_norms(oracle, indptr, values, block=8192):
    """rinv and zero flags of every row from oracle.normalize on left-packed rows (a row's stored values in order,
    then zeros: the same chain)."""
    n = indptr.size - 1
    rinv = np.empty(n, np.float32)
    zero = np.empty(n, np.uint8)
    lens = np.diff(indptr)
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        w = max(1, int(lens[r0:r1].max()))
        X = np.zeros((r1 - r0, w), np.float32)
        rr = np.repeat(np.arange(r1 - r0), lens[r0:r1])
        cc = np.arange(indptr[r0], indptr[r1]) - np.repeat(indptr[r0:r1], lens[r0:r1])
        X[rr, cc] = values[indptr[r0]:indptr[r1]]
        _, rinv[r0:r1], zero[r0:r1] = oracle.normalize(X)
    return rinv, zero


def _check_queries(oracle, indptr, indices, values, F, k, rows, got):
    """Each query against every row restricted to the query's own features (the only terms its chains have)."""
    n = indptr.size - 1
    rinv, zero = _row_norms(oracle, indptr, values)
    A = sp.csr_matrix((values, indices, indptr), shape=(n, F)).tocsc()
    for q in rows:
        cols = indices[indptr[q]:indptr[q + 1]]
        if cols.size == 0:
            T = np.zeros((n, 1), np.float32)
        else:
            T = A[:, cols].toarray().astype(np.float32)
        Th = (T * rinv[:, None]).astype(np.float32)
        wi, wd = oracle.knn_normalized(Th[q:q + 1], zero[q:q + 1], Th, zero, k)
        assert np.array_equal(got[0][q], wi[0]), "row %d: %s vs %s" % (q, got[0][q], wi[0])
        assert np.array_equal(got[1][q].view(np.uint32), wd[0].view(np.uint32)), "row %d distances" % q


def _heavy_rows(n, seed):
    """Feature 0 in every row, a few medium features (df ~ n / 50) and private-ish light ones."""
    rng = np.random.default_rng(seed)
    rows, vals = [], []
    for i in range(n):
        ids = {0, 1 + int(rng.integers(0, 50)), 100 + int(rng.integers(0, 5000))}
        if i % 3 == 0:
            ids.add(6000 + int(rng.integers(0, 100000)))
        ids = np.array(sorted(ids), np.int64)
        rows.append(ids)
        vals.append((rng.integers(1, 8, size=ids.size) * 0.25).astype(np.float32))
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    return indptr, np.concatenate(rows).astype(np.int32), np.concatenate(vals)


def test_heavy_postings_take_the_range_split(ctx, oracle):
    n, F, k = 50000, 1 << 24, 20
    indptr, indices, values = _heavy_rows(n, seed=5)
    got = ctx.knn_sparse(indptr, indices, values, F, k)
    t = ctx.last_knn_trace()
    assert t["kind"] == "sparse" and t["range_queries"] > 0 and t["range_chunks"] > 1, t
    rng = np.random.default_rng(3)
    rows = np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), rng.choice(n, 40, replace=False)]))
    _check_queries(oracle, indptr, indices, values, F, k, rows, got)


def _synth_idf(R, seed=602):
    from fedrann_amd.precompute import idf_weights
    from fedrann_amd.synth import synth
    s = synth(R, seed=seed, doubling=True)
    idf = idf_weights(s["counts"], s["n_features"])
    return s["indptr"], s["indices"], idf[s["indices"]], s["n_features"]


def test_synthetic_reads_at_scale(ctx, oracle):
    indptr, indices, values, F = _synth_idf(100_000)
    n, k = indptr.size - 1, 20
    got = ctx.knn_sparse(indptr, indices, values, F, k)
    assert ctx.last_knn_trace()["kind"] == "sparse"
    rng = np.random.default_rng(11)
    rows = np.unique(np.concatenate([np.arange(4), np.arange(n - 4, n), rng.choice(n, 120, replace=False)]))
    _check_queries(oracle, indptr, indices, values, F, k, rows, got)


def test_nndescent_on_a_wide_csr(ctx):
    """A csr_matrix with F = 1.3 M columns: NNDescent_ava searches it sparse (densifying it would need n x F floats)."""
    from fedrann_amd.nearest_neighbors import NNDescent_ava
    indptr, indices, values, _ = _hard_rows(6000, seed=21, F=1_300_000, n_ids=1500)
    A = sp.csr_matrix((values, indices, indptr), shape=(6000, 1_300_000))
    got = NNDescent_ava().get_neighbors(A, index_n_neighbors=20, context=ctx, verbose=False)
    want = ctx.knn_sparse(indptr, indices, values, 1_300_000, 20)
    _same(got, want)


def test_nndescent_narrow_csr_keeps_the_dense_route(ctx):
    """<= FDR_MAX_DIM columns: the dense route, as before, and the same bits as the sparse search."""
    from fedrann_amd.nearest_neighbors import NNDescent_ava
    indptr, indices, values, _ = _hard_rows(4000, seed=22, F=1024, n_ids=1024)
    A = sp.csr_matrix((values, indices, indptr), shape=(4000, 1024))
    got = NNDescent_ava().get_neighbors(A, index_n_neighbors=20, context=ctx, verbose=False)
    assert ctx.last_knn_trace()["kind"] != "sparse"
    _same(got, ctx.knn_sparse(indptr, indices, values, 1024, 20))


def _run_cli(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "fedrann_amd"] + args, cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=timeout)


def test_cli_no_projection_from_a_feature_matrix(ctx, tmp_path):
    from fedrann_amd.__main__ import write_overlaps
    from fedrann_amd.feature_extraction import save_feature_matrix_npz
    from fedrann_amd.precompute import idf_weights
    from fedrann_amd.synth import synth
    s = synth(3000, seed=44, doubling=True)
    fm, cnt = str(tmp_path / "feature_matrix.npz"), str(tmp_path / "counts.npy")
    save_feature_matrix_npz(fm, s["indptr"], s["indices"], s["n_features"])
    np.save(cnt, s["counts"])
    out = tmp_path / "out"
    r = _run_cli(["-o", str(out), "--feature-matrix", fm, "--kmer-counts", cnt, "--no-projection",
                  "--nndescent-n-neighbors", "20"])
    assert r.returncode == 0, r.stderr[-3000:]
    idf = idf_weights(s["counts"], s["n_features"])
    idx, dist = ctx.knn_sparse(s["indptr"], s["indices"], idf[s["indices"]], s["n_features"], 20)
    want = tmp_path / "want.tsv"
    n = s["indptr"].size - 1
    write_overlaps(str(want), idx, dist, ["row_%d" % i for i in range(n)], [0] * n)  # (no --read-names)
    assert (out / "overlaps.tsv").read_bytes() == want.read_bytes()


def test_cli_no_projection_refuses_devices(tmp_path):
    r = _run_cli(["-o", str(tmp_path / "out"), "--feature-matrix", "x.npz", "--kmer-counts", "c.npy",
                  "--no-projection", "--devices", "0,1"], timeout=120)
    assert r.returncode != 0
    assert "--no-projection" in r.stderr and "--devices" in r.stderr
