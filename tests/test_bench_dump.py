"""bench.py --dump-outputs (CPU only): what the last timed step returned, as float32 / float64 .npy files of at most
64 MB, every row when they fit and otherwise the same seeded sample of rows on every run."""
import os

import numpy as np
import pytest
import torch

import bench


def _step_result(n, k, d):
    """A stand-in for ShardedPipeline.step's (idx, dist, E) whose every entry names its row (broadcast views: no
    n x d allocation)."""
    r = torch.arange(n, dtype=torch.int32)[:, None]
    return r.expand(n, k), (r.float() / n).expand(n, k), (r.float() * 0.5).expand(n, d)


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}


def _check(got, n, k, d):
    assert set(got) == {"rows", "indices", "distances", "embedding"}
    assert got["rows"].dtype == np.float64 and got["indices"].dtype == np.float64
    assert got["distances"].dtype == np.float32 and got["embedding"].dtype == np.float32
    rows = got["rows"]
    m = rows.size
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert got["indices"].shape == (m, k) and got["distances"].shape == (m, k) and got["embedding"].shape == (m, d)
    assert np.array_equal(got["indices"], np.repeat(rows[:, None], k, 1))
    assert np.array_equal(got["distances"], np.repeat((rows.astype(np.float32) / np.float32(n))[:, None], k, 1))
    assert np.array_equal(got["embedding"], np.repeat((rows.astype(np.float32) * np.float32(0.5))[:, None], d, 1))
    return rows


def test_dump_writes_every_row_when_it_fits(tmp_path):
    n, k, d = 1000, 20, 128
    bench.dump_outputs(str(tmp_path / "a"), _step_result(n, k, d), 0, n, k, d, 1, 0)
    rows = _check(_load(str(tmp_path / "a")), n, k, d)
    assert np.array_equal(rows, np.arange(n))


@pytest.mark.parametrize("n,k,d", [(3_000_000, 20, 128), (20_000_000, 50, 256)])
def test_dump_samples_the_same_rows_within_64_mb(tmp_path, n, k, d):
    out = _step_result(n, k, d)
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), out, 0, n, k, d, 1, 0)
        total = sum(os.path.getsize(os.path.join(str(tmp_path / tag), f)) for f in os.listdir(str(tmp_path / tag)))
        assert total <= bench.DUMP_BYTES <= 64 * 2**20
    a, b = _check(_load(str(tmp_path / "a")), n, k, d), _check(_load(str(tmp_path / "b")), n, k, d)
    assert np.array_equal(a, b) and 0.9 * bench.DUMP_BYTES <= a.size * (8 + 12 * k + 4 * d) and a.size < n
