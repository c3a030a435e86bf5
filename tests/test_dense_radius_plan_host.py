"""The target chunks of the dense radius search (radius_chunks / radius_chunk_rows, csrc/knn_plan.inc) against the
planner, on the host: tests/dense_radius_plan/plan_check.cpp, a stand-alone program built with the address and
undefined-behaviour sanitizers, plans every chunk of index sizes on both sides of 96 << 19 = 50 331 648 rows (what one
plan of the fp16 shapes holds) up to 2^31 - 1 and fails where a plan has more than FDR_MAX_SEG segments, a segment
longer than 2^19 rows, or the chunks do not cover the index once."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "dense_radius_plan", "plan_check.cpp")
ONE_PLAN = 96 << 19
SIZES = [1, 31, 4097, ONE_PLAN - 1, ONE_PLAN, ONE_PLAN + 1, 60_000_000, 2 * ONE_PLAN, 2 * ONE_PLAN + 1, 2 ** 31 - 1]


def test_every_chunk_fits_one_plan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    binary = str(tmp_path / "plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wno-unused-function", "-pthread",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", binary], check=True)
    r = subprocess.run([binary] + [str(n) for n in SIZES], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert [row[0] for row in rows] == SIZES
    for n, chunks, chunk_rows, max_nseg in rows:
        assert chunks == -(-n // ONE_PLAN) and chunk_rows <= ONE_PLAN and chunk_rows % 32 == 0
        assert chunks * chunk_rows >= n > (chunks - 1) * chunk_rows and 1 <= max_nseg <= 96
    assert rows[SIZES.index(ONE_PLAN)][1] == 1 and rows[SIZES.index(ONE_PLAN + 1)][1] == 2  # the boundary itself
