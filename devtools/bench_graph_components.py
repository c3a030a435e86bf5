"""Time Context.graph_components (fdr_graph_components, host to host: the host's indptr pass, the upload, the pack
kernel and the segmented sort by index, the union-find's link, flatten and label kernels and one scan, the labels and
sizes back) beside graph.component_labels (numpy + scipy behind the rule check) and beside a bare
scipy.sparse.csgraph.connected_components on the same graph, in the same process, for both modes; and beside
Context.graph_symmetrize union on the same graph, for scale.

    python devtools/bench_graph_components.py [--shape knn100k knn1m ragged100k] [--mode union mutual]
                                              [--distance D] [--reps 5] [--numpy-reps 1]

Shapes: those of devtools/bench_graph_symmetrize.py (k-NN-like graphs of 100 000 x 20 and 1 000 000 x 20 with half of
every row's pairs reciprocated, a ragged one of 100 000 rows of about 100 entries).  The union graphs are one component
or nearly so, which makes them the measurement of the link kernel's contention and of the flatten kernel's aggregated
count; --distance cuts them apart (the distances are uniform in [0, 1)).  One warm-up call, then --reps timed ones:
median (min - max).  The labels and sizes are checked against the model, array for array.  The kernels alone are not
timed here (the library has no timing slot for them): take one `rocprofv3 --kernel-trace --stats` run of this script
with one --shape, one --mode, --numpy-reps 0 and --no-symmetrize, and read the gs_pack_kernel, gc_*_kernel and rocprim
rows; the same run without --no-symmetrize puts the symmetrise's gs_*_kernel rows beside them."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_graph_symmetrize import SHAPES, timed  # noqa: E402
from fedrann_amd import _lib  # noqa: E402
from fedrann_amd.graph import component_labels  # noqa: E402

MODES = ("union", "mutual")


def scipy_components(n, ip, ix, ds, mode, bound):
    """the number of components by scipy alone: no rule check, no relabelling"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    a = csr_matrix((np.ones(ix.size, np.int8) if bound is None else (ds <= np.float32(bound)).astype(np.int8), ix, ip),
                   shape=(n, n))
    if mode == "mutual":
        if bound is None:
            a = a.multiply(a.T)
        else:  # each lists the other, and the smaller distance is within the bound: either direction's is
            listed = csr_matrix((np.ones(ix.size, np.int8), ix, ip), shape=(n, n))
            a = listed.multiply(listed.T).multiply(a + a.T)
    a = csr_matrix(a, copy=True)  # (not the caller's arrays: the next line edits in place)
    a.eliminate_zeros()  # (csgraph takes a stored zero for a link)
    return connected_components(a, directed=False, return_labels=False)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", nargs="+", choices=sorted(SHAPES), default=["knn100k", "knn1m", "ragged100k"])
    ap.add_argument("--mode", nargs="+", choices=MODES, default=list(MODES))
    ap.add_argument("--distance", type=float, default=None, help="the bound; by default every entry joins")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-reps", type=int, default=1, help="0: skip the numpy model, scipy and the comparison")
    ap.add_argument("--no-symmetrize", action="store_true", help="skip the graph_symmetrize union run")
    a = ap.parse_args()
    ok = True
    with _lib.Context(0) as ctx:
        for shape in a.shape:
            graph = SHAPES[shape]()
            _, n, ip, ix, ds = _lib.check_graph_symmetrize(graph)
            print("%s: %d rows, %d entries (%.1f MB up), %d reps" % (shape, n, ix.size, 8 * ix.size / 1e6, a.reps), flush=True)
            for mode in a.mode:
                got, med, lo, hi = timed(lambda: ctx.graph_components(graph, mode, a.distance), a.reps)
                line = "  %-7s %8d components, largest %8d   GPU, host to host: %8.2f ms (%.2f - %.2f)" % (
                    mode, got[1].size, int(got[1].max()), med, lo, hi)
                if a.numpy_reps:
                    want, nmed, nlo, nhi = timed(lambda: component_labels(ip, ix, ds, mode, a.distance), a.numpy_reps, warmup=0)
                    same = all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
                    count, smed, slo, shi = timed(lambda: scipy_components(n, ip, ix, ds, mode, a.distance), a.numpy_reps,
                                                  warmup=0)
                    ok = ok and same and count == got[1].size
                    line += "   model: %9.1f ms (%.1f - %.1f)   scipy alone: %8.1f ms (%.1f - %.1f)   the same: %s" % (
                        nmed, nlo, nhi, smed, slo, shi, same and count == got[1].size)
                print(line, flush=True)
            if not a.no_symmetrize:
                sym, med, lo, hi = timed(lambda: ctx.graph_symmetrize(graph, "union", max_entries=2 ** 31 - 1), a.reps)
                print("  graph_symmetrize union, %9d entries out   GPU, host to host: %8.2f ms (%.2f - %.2f)"
                      % (sym[1].size, med, lo, hi), flush=True)
            ctx.graph_free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
