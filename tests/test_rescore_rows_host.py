"""The parts of the held re-score rows (fdr_rescore_rows_*, `--radius R --radius-rescore METRIC`) that need no GPU: the
argument checks of RescoreRows.radius and the command line's refusals before any work."""
import numpy as np
import pytest

from fedrann_amd import __main__ as cli
from fedrann_amd import _lib


def _ragged(lens=(0, 3, 1, 0, 200)):
    ip = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ip[1:])
    return ip, np.zeros(int(ip[-1]), np.int32)


def test_check_rescore_ragged_accepts_a_valid_call():
    ip, ix = _ragged()
    nq, r, q_lo, counts = _lib.check_rescore_ragged(10, ip, ix, 0.25)
    assert (nq, q_lo) == (5, 0) and r == np.float32(0.25) and r.dtype == np.float32
    assert counts.dtype == np.int64 and list(counts) == [0, 3, 1, 0, 200]
    assert _lib.check_rescore_ragged(10, ip, ix, 1, q_lo=5)[:3] == (5, np.float32(1), 5)  # (1 keeps every candidate)
    assert _lib.check_rescore_ragged(10, ip, ix, 0.0)[1] == 0
    for minus_zero in (-0.0, np.float32(-0.0)):  # -0.0 is 0, and its sign bit does not reach the library
        r = _lib.check_rescore_ragged(10, ip, ix, minus_zero)[1]
        assert r.dtype == np.float32 and r.view(np.uint32) == 0
    assert _lib.check_rescore_ragged(10, ip, ix, np.float32(0.5))[1] == np.float32(0.5)
    nq, _, _, counts = _lib.check_rescore_ragged(10, np.zeros(1, np.int64), np.zeros(0, np.int32), 0.5, q_lo=10)
    assert nq == 0 and counts.size == 0
    assert _lib.check_rescore_ragged(10, np.zeros(4, np.int64), np.zeros(0, np.int32), 0.5)[0] == 3  # every row empty


def test_check_rescore_ragged_rejects_the_arrays():
    ip, ix = _ragged()
    with pytest.raises(TypeError, match="cand_indptr"):
        _lib.check_rescore_ragged(10, ip.astype(np.int32), ix, 0.5)
    with pytest.raises(TypeError, match="cand_idx"):
        _lib.check_rescore_ragged(10, ip, ix.astype(np.int64), 0.5)
    with pytest.raises(TypeError):
        _lib.check_rescore_ragged(10, ip.tolist(), ix, 0.5)
    with pytest.raises(ValueError, match="1-D"):
        _lib.check_rescore_ragged(10, ip.reshape(2, 3), ix, 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        _lib.check_rescore_ragged(10, ip, np.zeros(2 * ix.size, np.int32)[::2], 0.5)
    with pytest.raises(ValueError):
        _lib.check_rescore_ragged(10, np.zeros(0, np.int64), np.zeros(0, np.int32), 0.5)  # not even indptr[0]
    with pytest.raises(ValueError, match="must hold"):
        _lib.check_rescore_ragged(10, ip, ix[:-1], 0.5)


def test_check_rescore_ragged_rejects_the_indptr():
    ip, ix = _ragged()
    off = ip.copy()
    off[0] = 1
    with pytest.raises(ValueError, match="start at 0"):
        _lib.check_rescore_ragged(10, off, ix, 0.5)
    down = ip.copy()
    down[3] = down[2] - 1
    with pytest.raises(ValueError, match="decreases at query 5"):
        _lib.check_rescore_ragged(10, down, ix, 0.5, q_lo=3)
    huge = np.array([0, 1 << 31], np.int64)
    with pytest.raises(ValueError, match="2\\^31"):
        _lib.check_rescore_ragged(10, huge, ix, 0.5)


def test_check_rescore_ragged_rejects_the_radius():
    ip, ix = _ragged()
    for radius in (float("nan"), -0.1, 1.5, np.nextafter(np.float32(1), np.float32(2))):
        with pytest.raises(ValueError, match="radius"):
            _lib.check_rescore_ragged(10, ip, ix, radius)
    for radius in ("0.5", None, True):
        with pytest.raises(ValueError, match="number"):
            _lib.check_rescore_ragged(10, ip, ix, radius)


def test_check_rescore_ragged_rejects_the_window():
    ip, ix = _ragged()
    with pytest.raises(ValueError, match="range"):
        _lib.check_rescore_ragged(10, ip, ix, 0.5, q_lo=6)  # q_lo + nq = 11 > n
    with pytest.raises(ValueError, match="range"):
        _lib.check_rescore_ragged(10, ip, ix, 0.5, q_lo=-1)
    with pytest.raises(ValueError, match="range"):
        _lib.check_rescore_ragged(4, ip, ix, 0.5)
    with pytest.raises(ValueError, match="integer"):
        _lib.check_rescore_ragged(10, ip, ix, 0.5, q_lo=1.0)


BASE = ["--feature-matrix", "m.npz", "--kmer-counts", "c.npy"]


@pytest.mark.parametrize("extra, words", [
    (["--radius-rescore", "jaccard"], "needs --radius"),
    (["--radius", "0.5", "--radius-rescore-bound", "0.5"], "needs --radius-rescore"),
    (["--radius-rescore-bound", "0.5"], "needs --radius-rescore"),
    (["--radius", "0.5", "--radius-rescore", "cosine", "--radius-rescore-bound", "1.5"], "[0, 1]"),
    (["--radius", "0.5", "--radius-rescore", "cosine", "--radius-rescore-bound", "-0.1"], "[0, 1]"),
    (["--radius", "0.5", "--radius-rescore", "cosine", "--radius-rescore-bound", "nan"], "[0, 1]"),
    (["--radius", "0.5", "--radius-rescore", "jaccard", "--no-projection"], "--no-projection"),
    (["--radius-rescore", "jaccard", "--no-projection"], "exact already"),
    (["--radius", "0.5", "--radius-rescore", "weighted_jaccard", "--devices", "0,1"], "one GPU"),
    (["--radius", "0.5", "--radius-rescore", "jaccard", "--rescore", "jaccard"], "--radius"),
])
def test_cli_refuses_before_any_work(tmp_path, extra, words):
    out_dir = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        cli.main(["-o", str(out_dir)] + BASE + extra)
    assert words in str(e.value), e.value
    assert not out_dir.exists()  # (before any work: not even the output directory)


def test_check_radius_rescore_passes_what_is_fine():
    parse = cli.parse_command_line_arguments
    assert cli.check_radius_rescore(parse(["-o", "x"] + BASE)) is None
    assert cli.check_radius_rescore(parse(["-o", "x", "--radius", "0.5"] + BASE)) is None
    assert cli.check_radius_rescore(parse(["-o", "x", "--radius", "0.5", "--radius-rescore", "jaccard"] + BASE)) == 1.0
    assert cli.check_radius_rescore(parse(["-o", "x", "--radius", "0.5", "--radius-rescore", "cosine",
                                           "--radius-rescore-bound", "0.25", "--devices", "0"] + BASE)) == 0.25
    assert cli.check_radius_rescore(parse(["-o", "x", "--radius", "0.5", "--radius-rescore", "weighted_jaccard",
                                           "--radius-rescore-bound", "0"] + BASE)) == 0.0
    import math
    r2 = cli.check_radius_rescore(parse(["-o", "x", "--radius", "0.5", "--radius-rescore", "jaccard",
                                         "--radius-rescore-bound=-0.0"] + BASE))
    assert r2 == 0.0 and math.copysign(1.0, r2) == 1.0  # (-0.0 is 0)


def test_the_fixture_has_the_edges():
    """the rows and candidate lists of tests/test_gpu_rescore_rows.py hold the lane, tile and batch edges they are for"""
    import _rescore_rows as rr
    lens = np.diff(rr.rows()[0])
    assert tuple(lens[:len(rr.SPECIAL)]) == rr.SPECIAL and lens[60] == 2 * rr.T + 3
    clens = np.diff(rr.ragged(rr.edge_lists())[0])
    assert set(rr.EDGE_LENGTHS) <= set(int(c) for c in clens)
    assert clens[rr.LONGEST] > _lib.FDR_MAX_K and clens[60] > 2 * _lib.FDR_MAX_K  # carried across tiles, in several batches
