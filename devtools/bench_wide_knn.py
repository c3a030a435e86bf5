"""Time fdr_knn_dev on synthetic normalised rows for k-NN calls beyond k <= 64 (the exact MFMA pass of knn_route):
    PYTHONPATH=. python devtools/bench_wide_knn.py N:d:k [N:d:k ...] [--reps R] [--warmup W]
Rows: fedrann_amd/synth.py reads -> projection -> embed -> normalise.  One JSON line per case: device-event ms per
call (median), flop = 2 * N^2 * dp, the fraction of the 157.3 TF fp32 matrix peak, and the kernel shape the trace
reports."""
import argparse
import json

import numpy as np
import torch

from fedrann_amd import _lib
from fedrann_amd.distributed import HipEngine
from fedrann_amd.precompute import build_precompute_matrix
from fedrann_amd.synth import synth

PEAK_FP32_MATRIX = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="+", help="N:d:k")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=0)
    ap.add_argument("--seed", type=int, default=602)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    with _lib.Context(0) as ctx:
        eng = HipEngine(ctx, dev)
        for case in args.cases:
            n, d, k = (int(x) for x in case.split(":"))
            s = synth(n, seed=args.seed, threads=16)
            P = build_precompute_matrix(s["counts"], d)
            ctx.projection_load(P.indptr, P.indices, P.data, s["n_features"], d)
            E = torch.from_numpy(ctx.embed(s["indptr"], s["indices"])).to(dev)
            del s
            dp = ctx.padded_dim(d)
            Ehat = torch.empty((n, dp), dtype=torch.float32, device=dev)
            zero = torch.empty((n,), dtype=torch.uint8, device=dev)
            eng.normalize(E, Ehat, zero)
            del E
            need = ctx.knn_workspace_bytes(n, n, d, k)
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
            idx = torch.empty((n, k), dtype=torch.int32, device=dev)
            dst = torch.empty((n, k), dtype=torch.float32, device=dev)
            st = torch.cuda.current_stream(dev)
            ms = []
            for rep in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                ctx.knn_dev(Ehat.data_ptr(), zero.data_ptr(), n, Ehat.data_ptr(), zero.data_ptr(), n, 0, d, k,
                            idx.data_ptr(), dst.data_ptr(), ws.data_ptr(), ws.numel(), st.cuda_stream)
                e1.record(st)
                e1.synchronize()
                if rep >= args.warmup:
                    ms.append(e0.elapsed_time(e1))
            tr = ctx.last_knn_trace()
            t = float(np.median(ms))
            flop = 2.0 * n * n * dp
            print(json.dumps({"N": n, "d": d, "dp": dp, "k": k, "ms": round(t, 3), "flop": flop,
                              "frac_fp32_peak": round(flop / (t * 1e-3) / PEAK_FP32_MATRIX, 4), "reps": len(ms),
                              "kind": tr["kind"], "generic": tr["generic"], "exact_waves": tr["exact_waves"],
                              "exact_qsets": tr["exact_qsets"], "workspace_bytes": need}), flush=True)
            del Ehat, zero, ws, idx, dst
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
