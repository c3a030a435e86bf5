"""The schedule of the live-chunk pass's end (live_issue_order and round_ready_points in knn_plan.inc; fdr_set_pass_tail),
built HOST-ONLY with AddressSanitizer + UBSan (the flags of test_host_san.py) and driven through
tests/host_san/pass_tail.cpp.  CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_san", "pass_tail.cpp")
BIN = os.path.join(HERE, "host_san", "pass_tail")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-pthread"]


def test_pass_tail_schedule_under_sanitizers():
    """For random plans -- with and without groups that join the next larger NL, only dense blocks, no dense block --
    the descending issue order is the plan's groups reversed (the dense group first, NL strictly falling); and for the
    launches of those groups on one and two queues a group's merge + re-rank is queued behind every launch of the
    group and in front of a later one, never for the group issued last: right behind its last launch (trigger GROUP:
    every group but the last), or in front of the queues' final launches for the groups complete by then (trigger
    LAST).  A plan of one group has nothing early.  Two lists spelled out by hand."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    csrc = os.path.join(os.path.dirname(HERE), "fedrann_amd", "csrc")
    deps = [SRC, os.path.join(csrc, "knn_plan.inc"), os.path.join(csrc, "host_common.inc")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.run([gxx] + FLAGS + [SRC, "-o", BIN], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    f = dict(kv.split("=", 1) for kv in r.stdout.split() if "=" in kv)
    assert f["rc"] == "0" and int(f["plans"]) == 400
    assert int(f["joined"]) > 10 and int(f["early"]) > 400 and int(f["late_only"]) > 20, f
