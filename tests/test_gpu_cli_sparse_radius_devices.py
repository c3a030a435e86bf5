"""`--no-projection --no-projection-radius R` over several `--devices` with `--sparse-shard targets`: each rank indexes
its own rows, the ranks' ragged rows are merged on the GPU (distributed.sparse_radius_sharded), and overlaps.tsv is the
single-GPU command line's file byte for byte.  The ranks share GPU 0 over gloo (RCCL needs one GPU per rank)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from test_gpu_cli_sparse_radius import _inputs

pytestmark = pytest.mark.gpu


def _run_cli(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "fedrann_amd"] + args, cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=timeout)


@pytest.mark.parametrize("metric", ["jaccard", "cosine"])
def test_sharded_radius_file_is_the_single_gpu_file(tmp_path, metric):
    _, inputs = _inputs(tmp_path)
    base = inputs + ["--no-projection", "--no-projection-metric", metric, "--no-projection-radius", "0.9"]
    one = _run_cli(["-o", str(tmp_path / "one")] + base)
    assert one.returncode == 0, one.stderr[-3000:]
    many = _run_cli(["-o", str(tmp_path / "many"), "--devices", "0,0,0", "--dist-backend", "gloo", "--sparse-shard",
                     "targets", "--keep-intermediates"] + base)
    assert many.returncode == 0, many.stderr[-3000:]
    want = (tmp_path / "one" / "overlaps.tsv").read_bytes()
    assert len(want) > 100_000 and (tmp_path / "many" / "overlaps.tsv").read_bytes() == want
    parts = sorted(p.name for p in (tmp_path / "many" / "temp").iterdir() if p.name.startswith("overlaps.rank"))
    assert parts == ["overlaps.rank%d.tsv" % r for r in range(3)]
    assert all((tmp_path / "many" / "temp" / p).stat().st_size > 0 for p in parts)
