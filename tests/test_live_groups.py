"""The grouping of the d <= 128 candidate pass's query blocks by live chunks (live_plan in knn_plan.inc), built HOST-ONLY
with AddressSanitizer + UBSan (the flags of test_host_san.py) and driven through tests/host_san/live_groups.cpp.  CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_san", "live_groups.cpp")
BIN = os.path.join(HERE, "host_san", "live_groups")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-pthread"]


def test_live_chunk_groups_under_sanitizers():
    """Given the blocks' chunk masks: every block appears exactly once; a group's blocks ascend, so its work items
    (segment, block) are segment-major; a block runs on the instance of its own live-chunk count (below two: two) or,
    where its group is smaller than one launch, on the next larger one -- never a smaller one, and never moved when
    nothing is merged; the dense group holds exactly the blocks of seven or eight live chunks (plus a last live group too
    small for a launch); a block's ids are its group's NL chunks, ascending, and cover its mask.

    And the launches round_schedule (knn_plan.inc) deals for every such plan's groups and for a single group of the same
    blocks, launch sizes 0, 1, 64, 512 on 1, 2 and 4 queues: each group's items covered exactly once by launches with
    ascending, contiguous base, groups in the plan's order, no launch above the launch size, only a group's last launch
    short, launch i on queue i mod queues, launch size 0 one launch per non-empty group; one list spelled out by hand."""
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
    assert f["rc"] == "0" and int(f["plans"]) > 200 and int(f["merged"]) > 100
    assert int(f["schedules"]) >= 2 * 12 * int(f["plans"])  # (every plan: its groups and the single group, 4 sizes x 3 queues)
