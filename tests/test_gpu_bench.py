"""bench.py end to end on the GPU at config 2's size (100 k reads, seconds per run): a plain run prints the headline line
and runs nothing else; --full adds the other-mode pass, the host-to-host passes, the CPU baseline and recall, each
checked against the timed run's results."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--reads", "100000", "--steps", "2", "--warmup", "1"]
                       + list(args), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_plain_line():
    j = _bench()
    assert j["full"] is False and j["value"] > 0 and j["ms_per_step"] > 0 and j["config"]["self_check"]
    assert j["kernels_ms"]["knn_prefilter"] > 0 and j["roofline"]["achieved"] > 0
    assert "other_mode" not in j and j["host_to_host"] is None and j["value_host_to_host"] is None
    assert j["cpu_baseline"] is None and j["recall"] is None and j["roofline"]["traffic"] is None


def test_bench_full_line():
    j = _bench("--full", "--cpu-baseline-seconds", "1")
    assert j["full"] is True and j["value"] > 0 and j["config"]["self_check"]
    assert j["other_mode"]["mode"] == "exact" and j["other_mode"]["identical_to_timed_run"]
    assert all(j["host_to_host"][c]["identical_to_timed_run"] for c in ("full_csr", "compacted_csr"))
    assert j["value_host_to_host"] == j["host_to_host"]["full_csr"]["value"] > 0
    assert j["recall"]["ranks_and_distance_bits_identical"] and j["recall"]["recall_vs_oracle"] == 1.0
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["nndescent"]["rows"] > 0
