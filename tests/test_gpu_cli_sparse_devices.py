"""`--no-projection` over several `--devices`: with `--sparse-shard targets` (each rank loads and indexes its own rows,
distributed.sparse_knn_sharded) and with `--sparse-shard queries` (each rank indexes all rows and searches its own)
overlaps.tsv is the single-GPU command line's file byte for byte; without the flag the run is refused and told of it.
The ranks share GPU 0 over gloo (RCCL needs one GPU per rank)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from fedrann_amd.feature_extraction import save_feature_matrix_npz
from fedrann_amd.synth import synth

pytestmark = pytest.mark.gpu


def _run_cli(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "fedrann_amd"] + args, cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=timeout)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("inputs")
    s = synth(3000, seed=44, doubling=True)
    fm, cnt = str(d / "feature_matrix.npz"), str(d / "counts.npy")
    save_feature_matrix_npz(fm, s["indptr"], s["indices"], s["n_features"])
    np.save(cnt, s["counts"])
    return ["--feature-matrix", fm, "--kmer-counts", cnt, "--nndescent-n-neighbors", "20"]


@pytest.mark.parametrize("mode,devices,extra", [
    ("targets", "0,0,0", []),
    ("queries", "0,0", ["--no-projection-metric", "jaccard"]),
])
def test_sharded_file_is_the_single_gpu_file(inputs, tmp_path, mode, devices, extra):
    base = inputs + ["--no-projection"] + extra
    one = _run_cli(["-o", str(tmp_path / "one")] + base)
    assert one.returncode == 0, one.stderr[-3000:]
    sharded = base + ["--devices", devices, "--dist-backend", "gloo"]
    many = _run_cli(["-o", str(tmp_path / "many"), "--sparse-shard", mode, "--keep-intermediates"] + sharded)
    assert many.returncode == 0, many.stderr[-3000:]
    want = (tmp_path / "one" / "overlaps.tsv").read_bytes()
    assert len(want) > 100_000 and (tmp_path / "many" / "overlaps.tsv").read_bytes() == want
    parts = sorted(p.name for p in (tmp_path / "many" / "temp").iterdir() if p.name.startswith("overlaps.rank"))
    assert parts == ["overlaps.rank%d.tsv" % r for r in range(len(devices.split(",")))]
    # the same invocation without the flag: refused before any work, and told which flag decides
    refused = _run_cli(["-o", str(tmp_path / "refused")] + sharded, timeout=120)
    assert refused.returncode != 0 and "--sparse-shard targets|queries" in refused.stderr
    assert "--no-projection" in refused.stderr and "--devices" in refused.stderr
    assert not (tmp_path / "refused").exists()


def test_targets_from_kmer_searcher_output(tmp_path):
    """The ranged loader's path: each rank reads its records of output.bin (600 records are 1200 rows: blocks of 416,
    416 and 368)."""
    from test_gpu_cli import _write_intermediates
    s = synth(600, seed=5, m=80)
    out_bin, fasta, _ = _write_intermediates(tmp_path, s, ["read_%d/ccs" % i for i in range(600)])
    base = ["--kmer-searcher-output", out_bin, "--kmer-library", fasta, "--nndescent-n-neighbors", "20",
            "--no-projection", "--no-projection-metric", "weighted_jaccard"]
    one = _run_cli(["-o", str(tmp_path / "one")] + base)
    assert one.returncode == 0, one.stderr[-3000:]
    many = _run_cli(["-o", str(tmp_path / "many"), "--sparse-shard", "targets", "--devices", "0,0,0", "--dist-backend",
                     "gloo"] + base)
    assert many.returncode == 0, many.stderr[-3000:]
    assert (tmp_path / "many" / "overlaps.tsv").read_bytes() == (tmp_path / "one" / "overlaps.tsv").read_bytes()


def test_targets_with_k_above_a_shard_is_refused_with_the_helpers_words(tmp_path):
    """40 records over three ranks leave the last one 16 rows, fewer than k = 20."""
    from test_gpu_cli import _write_intermediates
    s = synth(40, seed=5, m=80)
    out_bin, fasta, _ = _write_intermediates(tmp_path, s, ["r%d" % i for i in range(40)])
    short = _run_cli(["-o", str(tmp_path / "short"), "--sparse-shard", "targets", "--devices", "0,0,0", "--dist-backend",
                      "gloo", "--kmer-searcher-output", out_bin, "--kmer-library", fasta, "--nndescent-n-neighbors",
                      "20", "--no-projection"], timeout=300)
    assert short.returncode != 0
    assert "--sparse-shard targets: rank 2 of 3 holds 16 target rows" in short.stderr
    assert not (tmp_path / "short" / "overlaps.tsv").exists()
