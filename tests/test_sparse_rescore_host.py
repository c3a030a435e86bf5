"""The parts of the exact re-score (fdr_sparse_rescore, `--rescore`) that need no GPU: the argument checks of
Context.sparse_rescore, the command line's refusals before any work, and the default K' rule."""
import os

import numpy as np
import pytest

from fedrann_amd import __main__ as cli
from fedrann_amd import _lib


def _cands(nq=5, k_in=8, dtype=np.int32):
    return np.zeros((nq, k_in), dtype)


def test_check_rescore_args_accepts_a_valid_call():
    assert _lib.check_rescore_args(10, _cands()) == (5, 8, 8, 0)
    assert _lib.check_rescore_args(10, _cands(), k=3, metric="jaccard", q_lo=5) == (5, 8, 3, 5)
    out = (np.empty((5, 3), np.int32), np.empty((5, 3), np.float32))
    assert _lib.check_rescore_args(10, _cands(), k=3, metric="weighted_jaccard", out=out) == (5, 8, 3, 0)
    assert _lib.check_rescore_args(10, _cands(nq=0)) == (0, 8, 8, 0)
    assert _lib.check_rescore_args(7, _cands(nq=2, k_in=_lib.FDR_MAX_K), q_lo=5)[:2] == (2, _lib.FDR_MAX_K)


def test_check_rescore_args_rejects_k():
    with pytest.raises(ValueError, match="k_in"):
        _lib.check_rescore_args(10, _cands(), k=9)  # k_out > k_in
    with pytest.raises(ValueError):
        _lib.check_rescore_args(10, _cands(), k=0)
    with pytest.raises(ValueError, match="k_in"):
        _lib.check_rescore_args(10, _cands(k_in=_lib.FDR_MAX_K + 1))
    with pytest.raises(ValueError):
        _lib.check_rescore_args(10, _cands(k_in=0))
    with pytest.raises(ValueError):
        _lib.check_rescore_args(10, _cands(), k=2.0)


def test_check_rescore_args_rejects_the_candidate_array():
    with pytest.raises(TypeError):
        _lib.check_rescore_args(10, _cands(dtype=np.int64))
    with pytest.raises(TypeError):
        _lib.check_rescore_args(10, _cands().tolist())
    with pytest.raises(ValueError):
        _lib.check_rescore_args(10, np.zeros(8, np.int32))  # 1-D
    with pytest.raises(ValueError):
        _lib.check_rescore_args(10, np.zeros((5, 16), np.int32)[:, ::2])  # not contiguous
    with pytest.raises(ValueError, match="out"):
        _lib.check_rescore_args(10, _cands(), k=3, out=(np.empty((5, 8), np.int32), np.empty((5, 8), np.float32)))


def test_check_rescore_args_rejects_the_window():
    with pytest.raises(ValueError, match="range"):
        _lib.check_rescore_args(10, _cands(), q_lo=6)  # q_lo + nq = 11 > n
    with pytest.raises(ValueError, match="range"):
        _lib.check_rescore_args(10, _cands(), q_lo=-1)
    with pytest.raises(ValueError, match="range"):
        _lib.check_rescore_args(4, _cands())


def test_check_rescore_args_rejects_the_metric():
    with pytest.raises(ValueError, match="metric"):
        _lib.check_rescore_args(10, _cands(), metric="euclidean")
    with pytest.raises(ValueError, match="metric"):
        _lib.check_rescore_args(10, _cands(), metric=1)


def test_the_tile_constant_matches_the_header():
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "fedrann_hip.h")).read()
    assert int(re.search(r"#define FDR_RESCORE_TILE (\d+)", hdr).group(1)) == _lib.FDR_RESCORE_TILE


def test_default_candidates():
    assert cli.default_rescore_candidates(20) == 40
    assert cli.default_rescore_candidates(50) == 64
    assert cli.default_rescore_candidates(100) == 100
    assert cli.default_rescore_candidates(20, n=30) == 30  # capped by the reads there are


BASE = ["--feature-matrix", "m.npz", "--kmer-counts", "c.npy"]


@pytest.mark.parametrize("extra, words", [
    (["--rescore", "jaccard", "--no-projection"], "exact already"),
    (["--rescore", "cosine", "--radius", "0.5"], "--radius"),
    (["--rescore", "cosine", "--devices", "0,1"], "one GPU"),
    (["--rescore-candidates", "40"], "needs --rescore"),
    (["--rescore", "weighted_jaccard", "--nndescent-n-neighbors", "20", "--rescore-candidates", "19"],
     "--rescore-candidates must be in"),
    (["--rescore", "weighted_jaccard", "--nndescent-n-neighbors", "20", "--rescore-candidates", "129"],
     "--rescore-candidates must be in"),
])
def test_cli_refuses_before_any_work(tmp_path, extra, words):
    out_dir = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        cli.main(["-o", str(out_dir)] + BASE + extra)
    assert words in str(e.value), e.value
    assert not out_dir.exists()  # (before any work: not even the output directory)


def test_check_rescore_passes_what_is_fine():
    parse = cli.parse_command_line_arguments
    assert cli.check_rescore(parse(["-o", "x"] + BASE)) is None
    assert cli.check_rescore(parse(["-o", "x", "--rescore", "jaccard"] + BASE)) == 64  # (k = 50 by default)
    assert cli.check_rescore(parse(["-o", "x", "--rescore", "jaccard", "--nndescent-n-neighbors", "20"] + BASE)) == 40
    assert cli.check_rescore(parse(["-o", "x", "--rescore", "cosine", "--nndescent-n-neighbors", "20",
                                    "--rescore-candidates", "20", "--devices", "0"] + BASE)) == 20
    assert cli.check_rescore(parse(["-o", "x", "--rescore", "cosine", "--rescore-candidates", "128"] + BASE)) == 128
