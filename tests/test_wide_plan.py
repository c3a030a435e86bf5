"""The launch planner for k-NN calls beyond k <= 64 (knn_route / knn_plan in knn_plan.inc), built HOST-ONLY with
AddressSanitizer + UBSan (the flags of test_host_san.py) and driven through tests/host_san/wide_plan.cpp.  CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_san", "wide_plan.cpp")
BIN = os.path.join(HERE, "host_san", "wide_plan")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-pthread"]


def test_wide_knn_route_and_plans_under_sanitizers():
    """k <= 64 at d <= 512 keeps its passes; from 8192 targets, 64 < k <= 128 at d <= 512 and every k <= 128 at
    512 < d <= 1024 take the exact MFMA pass (everything else: the generic kernel).  Every such plan runs a release tile
    kernel of its dp (the split-K one at dp = 1024) with <= 128 queries per workgroup and >= 1 workgroup per CU in
    160 KiB of LDS, its segments are well formed (<= FDR_MAX_SEG, nseg * k keys within what the merge stages), and its
    partial lists are nseg * nq_pad * k * 8 bytes -- over target counts around 8192, 2^19, 1 M and 10 M, several
    query shares and 64 / 256 / 304 CUs."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    csrc = os.path.join(os.path.dirname(HERE), "fedrann_amd", "csrc")
    deps = [SRC, os.path.join(csrc, "knn_plan.inc"), os.path.join(csrc, "host_common.inc")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.run([gxx] + FLAGS + [SRC, "-o", BIN], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=900, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    f = dict(kv.split("=", 1) for kv in r.stdout.split() if "=" in kv)
    assert f["rc"] == "0" and int(f["plans"]) > 200 and int(f["wide"]) > 50 and int(f["generic"]) > 50
