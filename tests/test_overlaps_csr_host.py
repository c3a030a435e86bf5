"""The ragged overlaps writer (fdr_overlaps_write_csr): rows of one length give the fixed-width writer's bytes, ragged
rows the bytes of the writer's rule restated in plain Python, and the writer runs clean under AddressSanitizer + UBSan
in a stand-alone program (tests/host_san/overlaps_csr.cpp).  CPU only."""
import csv
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from fedrann_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = "query_name\tquery_orientation\ttarget_name\ttarget_orientation\tneighbor_rank\tdistance\n"


def _restated(indptr, idx, dist, names, strands, row0=0, header=True):
    """The rule of the writer: for row q = row0 + r and each entry c of the row, in order, unless its target t is q
    itself: name[q], strand[q], name[t], strand[t], c, dist -- c counts the skipped self entry, a negative t aliases
    from the end, the names go through csv.QUOTE_MINIMAL, float32 prints as numpy prints it.  strands=None: the
    names are those of the records of a doubled matrix, row t = record t >> 1 on strand t & 1."""
    n = len(names) * 2 if strands is None else len(names)
    name = (lambda t: names[t >> 1]) if strands is None else (lambda t: names[t])
    sign = (lambda t: "+-"[t & 1]) if strands is None else (lambda t: "+-"[strands[t]])
    buf = io.StringIO()
    w = csv.writer(buf, delimiter="\t", quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
    lines = 0
    for r in range(len(indptr) - 1):
        q = row0 + r
        for c, e in enumerate(range(indptr[r], indptr[r + 1])):
            t = int(idx[e])
            if t == q:
                continue
            if t < 0:
                t += n
            w.writerow([name(q), sign(q), name(t), sign(t), c, str(np.float32(dist[e]))])
            lines += 1
    return ((HEADER if header else "") + buf.getvalue()).encode(), lines


def _ragged(n, seed, n_targets=None):
    """Rows of 0 .. 8 entries: empty rows, self first, in the middle and last, negative indices, distances in both of
    the writer's layouts, exact 0 and inf."""
    rng = np.random.default_rng(seed)
    nt = n if n_targets is None else n_targets
    lens = rng.integers(0, 9, n)
    lens[rng.random(n) < 0.2] = 0
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    idx = rng.integers(0, nt, indptr[-1]).astype(np.int32)
    idx[rng.random(idx.size) < 0.02] = -1
    dist = rng.integers(0, 0x3f800000, idx.size, dtype=np.uint32).view(np.float32).copy()
    dist[rng.random(idx.size) < 0.05] = 0.0
    dist[rng.random(idx.size) < 0.02] = np.inf
    return indptr, idx, dist


def _put_self(indptr, idx, row0=0):
    """Self at the first, a middle and the last position of rows that have the room."""
    for r in range(indptr.size - 1):
        m = indptr[r + 1] - indptr[r]
        if m and r % 2 == 0:
            idx[indptr[r] + (0, m // 2, m - 1)[(r // 2) % 3]] = row0 + r


def test_rows_of_one_length_give_the_fixed_width_bytes(tmp_path):
    rng = np.random.default_rng(4)
    n, k = 9000, 12  # (large enough for the thread pool)
    idx = rng.integers(0, n, size=(n, k)).astype(np.int32)
    idx[::3, 0] = np.arange(n)[::3]
    idx[rng.random((n, k)) < 0.01] = -1
    dist = rng.integers(0, 0x3f800001, size=(n, k), dtype=np.uint32).view(np.float32).copy()
    names = ["r%d/%s" % (i // 2, "ab"[i % 2] * (i % 5)) for i in range(n)]
    off, buf8 = _lib.pack_names(names)
    strands = np.array([i % 2 for i in range(n)], np.uint8)
    indptr = k * np.arange(n + 1, dtype=np.int64)
    for threads in (1, 4):
        a, b = tmp_path / "fixed.tsv", tmp_path / "csr.tsv"
        la = _lib.overlaps_write(str(a), idx, dist, off, buf8, strands, n_threads=threads)
        lb = _lib.overlaps_write_csr(str(b), indptr, idx.ravel(), dist.ravel(), off, buf8, strands, n_threads=threads)
        assert la == lb > n * (k - 1) and a.read_bytes() == b.read_bytes()
    # a block of rows, appended, in the doubled-rows mode
    off2, buf2 = _lib.pack_names(names[:n // 2])
    la = _lib.overlaps_write(str(a), idx[:4000], dist[:4000], off2, buf2, None)
    la += _lib.overlaps_write(str(a), idx[4000:], dist[4000:], off2, buf2, None, row0=4000, append=True, header=False)
    lb = _lib.overlaps_write_csr(str(b), indptr[:4001], idx.ravel(), dist.ravel(), off2, buf2, None)
    lb += _lib.overlaps_write_csr(str(b), indptr[4000:] - indptr[4000], idx[4000:].ravel(), dist[4000:].ravel(), off2,
                                  buf2, None, row0=4000, append=True, header=False)
    assert la == lb and a.read_bytes() == b.read_bytes()


@pytest.mark.parametrize("doubled", [False, True])
def test_ragged_rows_give_the_restated_rule(tmp_path, doubled):
    n = 600
    indptr, idx, dist = _ragged(n, seed=5 + doubled)
    _put_self(indptr, idx)
    assert (np.diff(indptr) == 0).sum() > 50 and (idx == np.repeat(np.arange(n), np.diff(indptr))).sum() > 100
    if doubled:
        names = ["rec%d" % i for i in range(n // 2)]
        strands = None
    else:
        names = ["read_%d" % i for i in range(n)]
        strands = [int(i * 7 % 3 == 0) for i in range(n)]
    names[3], names[4], names[5] = 'tab\there', 'quo"te', "line\nfeed"
    off, buf8 = _lib.pack_names(names)
    want, lines = _restated(indptr, idx, dist, names, strands)
    p = tmp_path / "o.tsv"
    assert _lib.overlaps_write_csr(str(p), indptr, idx, dist, off, buf8, strands) == lines > n
    assert p.read_bytes() == want
    # the same rows in three appended blocks (row0 > 0), each with arrays of its own; the first block has no rows
    q = tmp_path / "parts.tsv"
    got = 0
    for i, (lo, hi) in enumerate(((0, 0), (0, 251), (251, n))):
        ip = np.ascontiguousarray(indptr[lo:hi + 1] - indptr[lo])
        part, part_lines = _restated(ip, idx[indptr[lo]:indptr[hi]], dist[indptr[lo]:indptr[hi]], names, strands,
                                     row0=lo, header=False)
        before = q.stat().st_size if i else 0
        made = _lib.overlaps_write_csr(str(q), ip, idx[indptr[lo]:indptr[hi]], dist[indptr[lo]:indptr[hi]], off, buf8,
                                       strands, row0=lo, append=i > 0, header=i == 0)
        assert made == part_lines and q.read_bytes()[before + (len(HEADER) if i == 0 else 0):] == part
        got += made
    assert got == lines and q.read_bytes() == want
    # an indptr that does not start at 0 addresses the arrays as they are
    r = tmp_path / "tail.tsv"
    tail, tail_lines = _restated(indptr[400:] - indptr[400], idx[indptr[400]:], dist[indptr[400]:], names, strands,
                                 row0=400)
    assert _lib.overlaps_write_csr(str(r), indptr[400:], idx, dist, off, buf8, strands, row0=400) == tail_lines
    assert r.read_bytes() == tail


def test_ragged_writer_refusals(tmp_path):
    indptr, idx, dist = _ragged(50, seed=9)
    off, buf8 = _lib.pack_names(["n%d" % i for i in range(50)])
    strands = np.zeros(50, np.uint8)
    p = str(tmp_path / "o.tsv")
    bad = idx.copy()
    bad[0] = 50
    with pytest.raises(_lib.FedrannHipError, match="overlaps_write_csr: row"):
        _lib.overlaps_write_csr(p, indptr, bad, dist, off, buf8, strands)
    with pytest.raises(ValueError, match="row pointer"):
        _lib.overlaps_write_csr(p, indptr[::-1].copy(), idx, dist, off, buf8, strands)
    with pytest.raises(ValueError, match="row pointer"):
        _lib.overlaps_write_csr(p, indptr + 1, idx, dist, off, buf8, strands)
    with pytest.raises(_lib.FedrannHipError, match="bad argument"):
        _lib.overlaps_write_csr(p, indptr, idx, dist, off, buf8, strands, row0=1)  # rows 1 .. 50 of 50
    L = _lib.load_library()
    rc = L.fdr_overlaps_write_csr(p.encode(), 0, 1, 50, 0, 50, None, idx.ctypes.data, dist.ctypes.data,
                                  off.ctypes.data, buf8.ctypes.data, strands.ctypes.data, 1, None)
    assert rc == _lib.FDR_E_ARG
    down = indptr.copy()
    down[7] = down[6] - 1 if down[6] > 0 else down[8] + 1
    rc = L.fdr_overlaps_write_csr(p.encode(), 0, 1, 50, 0, 50, down.ctypes.data, idx.ctypes.data, dist.ctypes.data,
                                  off.ctypes.data, buf8.ctypes.data, strands.ctypes.data, 1, None)
    assert rc == _lib.FDR_E_ARG and b"monotone" in L.fdr_last_error()


def test_ragged_writer_under_sanitizers(tmp_path):
    """tests/host_san/overlaps_csr.cpp: random ragged graphs with arrays sized exactly, whole and in appended blocks,
    both strand modes, the thread pool, the refusals."""
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed to build tests/host_san/overlaps_csr.cpp under the sanitizers"
    src = os.path.join(HERE, "host_san", "overlaps_csr.cpp")
    binary = os.path.join(HERE, "host_san", "overlaps_csr")
    csrc = os.path.join(os.path.dirname(HERE), "fedrann_amd", "csrc")
    deps = [src, os.path.join(csrc, "overlaps_writer.inc"), os.path.join(csrc, "host_common.inc")]
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-pthread",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if not os.path.exists(binary) or any(os.path.getmtime(d) > os.path.getmtime(binary) for d in deps):
        subprocess.run([gxx] + flags + [src, "-o", binary], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for threads in ("1", "4"):
        r = subprocess.run([binary, str(tmp_path), threads], capture_output=True, text=True, timeout=300, env=env)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
        f = dict(kv.split("=", 1) for kv in r.stdout.split() if "=" in kv)
        assert f["rc"] == "0" and int(f["cases"]) == 8 and int(f["lines"]) > 100000
