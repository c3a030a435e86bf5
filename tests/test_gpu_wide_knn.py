"""k-NN from 8192 targets with 64 < k <= 128 at d <= 512, or any k <= 128 at 512 < d <= 1024: the exact fp32 MFMA pass
(knn_route in knn_plan.inc; d > 512: the split-K kernel), not the generic kernel -- indices and distance bits against the oracle on sampled query rows, in every mode, through
fdr_knn_dev on a row block, at the 8192-target threshold and through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _guarded import knn_dev_guarded
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu


def _rows(n, d, seed):
    """Sparse rows with ties: all-zero rows, exact duplicates and scaled copies (as the generic kernel's test)."""
    rng = np.random.default_rng(seed)
    E = np.zeros((n, d), np.float32)
    nnz = 6
    cols = rng.integers(0, d, size=(n, nnz))
    vals = (rng.integers(1, 5, size=(n, nnz)) * 0.37 * rng.choice([-1.0, 1.0], size=(n, nnz))).astype(np.float32)
    np.put_along_axis(E, cols, vals, axis=1)
    E[::17] = 0.0
    E[5::40] = E[3]
    E[7::50] = 2.5 * E[4]
    return E


def _sample(n, seed, per=96):
    """Block edges plus random rows."""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([np.arange(0, 40), np.arange(n - 40, n), rng.choice(n, per, replace=False)])
    return np.unique(rows)


def _oracle_rows(oracle, E, k, rows):
    Eh, _, zero = oracle.normalize(E)
    return oracle.knn_normalized(Eh[rows], zero[rows], Eh, zero, k)


def _assert_rows_equal(got, want, rows):
    gi, gd = got
    wi, wd = want
    assert np.array_equal(gi[rows], wi)
    assert np.array_equal(gd[rows].view(np.uint32), wd.view(np.uint32))


def _assert_mfma_trace(ctx, n, dp, k):
    tr = ctx.last_knn_trace()
    assert tr["kind"] == "exact" and tr["generic"] == 0, tr
    assert tr["dp"] == dp and tr["k"] == k and tr["exact_calls"] == 1 and tr["exact_waves"] == 4, tr
    paths = ctx.last_query_paths(n)
    assert not np.any((paths & 0x7F) == _lib.PATH_GENERIC) and np.all(paths == _lib.PATH_EXACT)


@pytest.mark.parametrize("n,d,k", [(9000, 128, 100), (12000, 256, 128), (9000, 500, 65), (10000, 1000, 50),
                                   (8192, 1024, 128), (16384, 700, 100)])
def test_wide_knn_matches_oracle(ctx, oracle, n, d, k):
    E = _rows(n, d, n + d + k)
    got = ctx.knn(E, k)
    _assert_mfma_trace(ctx, n, ctx.padded_dim(d), k)
    rows = _sample(n, k)
    _assert_rows_equal(got, _oracle_rows(oracle, E, k, rows), rows)


@pytest.mark.parametrize("d,k", [(256, 100), (1000, 50)])
def test_wide_knn_same_bits_in_every_mode(ctx, oracle, d, k):
    """exact, prefilter and auto modes, and the duplicate-row layer forced on: the same bits, always the MFMA pass
    (d = 1000 with k <= 64 included: neither the prefilter nor the class layer applies there)."""
    n = 9000
    E = _rows(n, d, 77)
    results = []
    try:
        for mode, dedup in (("exact", "auto"), ("prefilter", "auto"), ("auto", "auto"), ("auto", "force"),
                            ("prefilter", "force")):
            ctx.set_knn_mode(mode)
            ctx.set_dedup_mode(dedup)
            results.append(ctx.knn(E, k))
            _assert_mfma_trace(ctx, n, ctx.padded_dim(d), k)
    finally:
        ctx.set_knn_mode("auto")
        ctx.set_dedup_mode("auto")
    for idx, dist in results[1:]:
        assert np.array_equal(idx, results[0][0])
        assert np.array_equal(dist.view(np.uint32), results[0][1].view(np.uint32))
    rows = _sample(n, 3)
    _assert_rows_equal(results[0], _oracle_rows(oracle, E, k, rows), rows)


@pytest.mark.parametrize("d", [500, 1000])
def test_wide_knn_dev_on_a_row_block(ctx, oracle, d):
    """fdr_knn_dev with the queries a ragged last block of the target rows and t_base != 0, in a workspace of exactly
    fdr_knn_workspace_bytes bytes."""
    import torch
    from fedrann_amd.distributed import HipEngine
    dev = torch.device("cuda", 0)
    n, k, t_base = 9000, 100, 1000
    dp = ctx.padded_dim(d)
    E = _rows(n, d, 5)
    eng = HipEngine(ctx, dev)
    Ehat = torch.zeros((n, dp), dtype=torch.float32, device=dev)
    zero = torch.zeros((n,), dtype=torch.uint8, device=dev)
    eng.normalize(torch.from_numpy(E).to(dev), Ehat, zero)
    Eh, _, ozero = oracle.normalize(E)
    for q0, q1 in ((0, 3008), (6016, 9000)):  # (the last of three 32-row-aligned blocks is ragged)
        nq = q1 - q0
        # (workspace and outputs hold 0xFF bytes between canaries, checked after the synchronise: tests/_guarded.py)
        idx, dst, _ = knn_dev_guarded(ctx, Ehat, zero, q0, nq, t_base, d, k,
                                      stream=torch.cuda.current_stream(dev).cuda_stream)
        _assert_mfma_trace(ctx, nq, dp, k)
        rows = q0 + _sample(nq, q0)
        wi, wd = oracle.knn_normalized(Eh[rows], ozero[rows], Eh, ozero, k)
        gi, gd = idx.cpu().numpy(), dst.cpu().numpy()
        assert np.array_equal(gi[rows - q0], wi + t_base)
        assert np.array_equal(gd[rows - q0].view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("d,k", [(128, 100), (1000, 20)])
def test_wide_knn_threshold_at_8192_targets(ctx, oracle, d, k):
    """8191 targets: the generic kernel; 8192: the MFMA pass.  Both give the oracle's bits."""
    E = _rows(8192, d, 8192)
    for n, kind in ((8191, "generic"), (8192, "exact")):
        got = ctx.knn(E[:n], k)
        tr = ctx.last_knn_trace()
        assert tr["kind"] == kind and tr["generic"] == (kind == "generic"), tr
        rows = _sample(n, n)
        _assert_rows_equal(got, _oracle_rows(oracle, E[:n], k, rows), rows)


@pytest.mark.parametrize("d", [500, 1000])
def test_cli_wide_k_from_kmer_searcher_output(tmp_path, oracle, d):
    """`-n 500 / 1000 --nndescent-n-neighbors 100` on 4100 records (8200 doubled rows): overlaps.tsv byte-equal to the oracle
    pipeline, and a two-rank --devices run over gloo byte-equal to the one-GPU file."""
    from fedrann_amd import __main__ as cli
    from fedrann_amd.synth import synth
    from test_gpu_cli import _write_intermediates
    s = synth(4100, seed=41, m=80)
    names = ["read_%d/ccs" % i for i in range(4100)]
    out_bin, fasta, L = _write_intermediates(tmp_path, s, names)
    base = ["-n", str(d), "--nndescent-n-neighbors", "100", "--kmer-searcher-output", out_bin, "--kmer-library", fasta]
    one = tmp_path / "one"
    cli.main(["-o", str(one)] + base)
    got = open(one / "overlaps.tsv", newline="").read()
    o_names, o_strands, o_rows = oracle.parse_output_bin(out_bin, L)
    P = oracle.precompute_matrix(s["counts"], d)
    indptr, indices = oracle.rows_to_csr(o_rows)
    E = oracle.embed(indptr, indices, P, 2 * L, d)
    idx, dist = oracle.knn(E, 100)
    assert got == oracle.overlaps_tsv(idx, dist, o_names, o_strands)
    many = tmp_path / "many"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "fedrann_amd", "-o", str(many), "--devices", "0,0", "--dist-backend",
                        "gloo"] + base, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (many / "overlaps.tsv").read_bytes() == (one / "overlaps.tsv").read_bytes()
