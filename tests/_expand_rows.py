"""A brute force of fdr_graph_expand's definition that shares nothing with fedrann_amd.graph.expand_rows: Python's own
sort of (distance bits, index) pairs and sets of indices, row by row."""
import numpy as np


def fan_rows(graph, fan):
    """[N_f(x) as a list of indices, in key order] for every row x"""
    ip, idx, dist = graph
    b = np.ascontiguousarray(dist, dtype=np.float32).view(np.uint32)
    out = []
    for x in range(ip.size - 1):
        row = sorted((int(b[e]), int(idx[e])) for e in range(int(ip[x]), int(ip[x + 1])))
        out.append([s for _, s in row[:fan]])
    return out


def brute(graph, fan, lo=0, hi=None):
    """The definition, row by row: (indptr int64, idx int32)."""
    near = fan_rows(graph, fan)
    hi = len(near) if hi is None else hi
    rows = []
    for r in range(lo, hi):
        found = set(near[r])
        for t in near[r]:
            found.update(s for s in near[t] if s != r)
        rows.append(sorted(found))
    out = np.zeros(hi - lo + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=out[1:])
    return out, np.array([s for r in rows for s in r], np.int32)


def same(got, want):
    """(indptr, idx) pairs, equal in dtype, shape and bytes"""
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
