"""Throughput of the W-way count merge of a sharded stage 1 (fdr_kmer_count_merge_dev) on device-resident runs:
    PYTHONPATH=. python devtools/bench_kmer_merge.py [W] [entries per run] [reps]
Bytes moved per call = the runs read once (16 B per entry) + the merged place of each entry written (code, total,
flag: 20 B) + the flags scanned (8 B) + the kept entries compacted (16 B each, read and written)."""
import sys
import time

import numpy as np
import torch

from fedrann_amd import _lib

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 22
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
rng = np.random.default_rng(1)
runs = [np.unique(rng.integers(0, 4 * n, size=n, dtype=np.uint64)) for _ in range(W)]  # (runs overlap heavily)
run_off = np.zeros(W + 1, dtype=np.int64)
np.cumsum([r.size for r in runs], out=run_off[1:])
M = int(run_off[-1])
codes = torch.from_numpy(np.concatenate(runs).view(np.int64)).cuda()
counts = torch.from_numpy(rng.integers(1, 4, size=M, dtype=np.int64)).cuda()
with _lib.Context(0) as ctx:
    st = torch.cuda.current_stream().cuda_stream
    kc, _ = ctx.kmer_count_merge_dev(run_off, codes.data_ptr(), counts.data_ptr(), 2, stream=st)  # (warm-up)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kc, _ = ctx.kmer_count_merge_dev(run_off, codes.data_ptr(), counts.data_ptr(), 2, stream=st)
        ts.append(time.perf_counter() - t0)
moved = M * (16 + 20 + 8) + kc.size * 32
t = float(np.median(ts))
print("W=%d entries=%d kept=%d  median %.3f ms per call (incl. the fetch to the host)  %.1f GB/s of %.2f GB moved"
      % (W, M, kc.size, t * 1e3, moved / t / 1e9, moved / 1e9))
