"""Symmetrise a neighbour graph in numpy: the statement fdr_graph_symmetrize (csrc/graph_symmetrize.inc) is held to, bit
for bit, and the route without a GPU.

A graph is square, on n rows, as ragged rows (indptr int64 [n + 1], idx int32, dist float32): an entry (t, d) of row q
says "q lists t at distance d", 0 <= t < n.  Rows need not be sorted; a self entry (q, q) is allowed and is its own
reverse.  Distances compare by their bit patterns read as uint32, b(q -> t), all at most 0x7f800000 (no sign, no NaN:
bit order is then value order).  Row r of the result holds s

    union      iff r lists s or s lists r, at the smaller bits of the directions present
    mutual     iff r lists s and s lists r, at min(b(r -> s), b(s -> r))
    transpose  iff s lists r, at b(s -> r)

and every row is strictly ascending by (distance bits, index), like every other ragged result of the package, so
_lib.overlaps_write_csr takes it as it is.  Refused (ValueError naming the smallest (row, rule), rules in this order):
an index outside [0, n); distance bits above 0x7f800000; an index listed twice in one row.
"""
import numpy as np

MODES = {"union": 0, "mutual": 1, "transpose": 2}  # include/fedrann_hip.h: FDR_GRAPH_*
MAX_BITS = 0x7f800000
RULES = ("an index outside [0, n)", "a distance that is negative or NaN (its bits must be at most 0x7f800000)",
         "an index listed twice")


def as_ragged(graph):
    """(idx int32 [n, k], dist float32 [n, k]) or (indptr int64 [n + 1], idx int32, dist float32) -> the ragged triple,
    C-contiguous; the rectangular pair is the ragged form with indptr = k * arange(n + 1).  ValueError for anything
    else: another length, dtype or shape, an indptr that does not start at 0, decreases or disagrees with idx."""
    try:
        graph = tuple(graph)
    except TypeError:
        raise ValueError("a graph is (idx [n, k], dist [n, k]) or (indptr, idx, dist)") from None
    if len(graph) not in (2, 3) or not all(isinstance(a, np.ndarray) for a in graph):
        raise ValueError("a graph is (idx [n, k], dist [n, k]) or (indptr, idx, dist), numpy arrays")
    idx, dist = graph[-2], graph[-1]
    if idx.dtype != np.int32 or dist.dtype != np.float32:
        raise ValueError("idx must be int32 and dist float32, got %s and %s" % (idx.dtype, dist.dtype))
    if len(graph) == 2:
        if idx.ndim != 2 or dist.shape != idx.shape:
            raise ValueError("a rectangular graph is idx and dist of one shape [n, k], got %s and %s"
                             % (idx.shape, dist.shape))
        n, k = idx.shape
        return (k * np.arange(n + 1, dtype=np.int64), np.ascontiguousarray(idx).reshape(-1),
                np.ascontiguousarray(dist).reshape(-1))
    indptr = graph[0]
    if indptr.dtype != np.int64:
        raise ValueError("indptr must be int64, got %s" % indptr.dtype)
    if indptr.ndim != 1 or idx.ndim != 1 or dist.ndim != 1 or indptr.size < 1:
        raise ValueError("a ragged graph is three 1-D arrays, indptr of n + 1 >= 1 elements")
    if indptr[0] != 0 or np.any(np.diff(indptr) < 0):
        raise ValueError("indptr must start at 0 and never decrease")
    if idx.size != indptr[-1] or dist.size != indptr[-1]:
        raise ValueError("idx (%d) and dist (%d) must hold the %d entries indptr states"
                         % (idx.size, dist.size, int(indptr[-1])))
    return np.ascontiguousarray(indptr), np.ascontiguousarray(idx), np.ascontiguousarray(dist)


def mode_code(mode):
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (", ".join(sorted(MODES)), mode))
    return MODES[mode]


def symmetrize_rows(indptr, idx, dist, mode):
    """The union / mutual / transposed rows of the ragged graph (indptr, idx, dist), see the module's docstring:
    (indptr int64 [n + 1], idx int32, dist float32), a function of the input alone."""
    code = mode_code(mode)
    indptr, idx, dist = as_ragged((indptr, idx, dist))
    n = indptr.size - 1
    if n < 1:
        raise ValueError("a graph has at least one row")
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    t = idx.astype(np.int64)
    bits = dist.view(np.uint32)
    # ---- the rules: the smallest (row, rule) ----
    by_index = np.lexsort((t, rows))  # every row ordered by index
    again = np.zeros(t.size, bool)
    again[1:] = (rows[by_index][1:] == rows[by_index][:-1]) & (t[by_index][1:] == t[by_index][:-1])
    broken = [rows[(t < 0) | (t >= n)], rows[bits > MAX_BITS], rows[by_index][again]]
    records = np.concatenate([r * 4 + rule for rule, r in enumerate(broken)])
    if records.size:
        worst = int(records.min())
        raise ValueError("row %d: %s" % (worst // 4, RULES[worst % 4]))
    # ---- the partner of (q -> t): (t -> q), found among the sorted pair codes ----
    pair = (rows * n + t)[by_index]  # ascending, distinct
    at = np.minimum(np.searchsorted(pair, t * n + rows), max(t.size - 1, 0))
    has = pair[at] == t * n + rows if t.size else np.zeros(0, bool)
    low = np.where(has, np.minimum(bits, bits[by_index][at]), bits) if t.size else bits
    if code == MODES["union"]:
        r, s, b = np.concatenate([rows, t[~has]]), np.concatenate([t, rows[~has]]), np.concatenate([low, bits[~has]])
    elif code == MODES["mutual"]:
        r, s, b = rows[has], t[has], low[has]
    else:
        r, s, b = t, rows, bits
    order = np.lexsort((s, b, r))  # rows in turn, each by (distance bits, index)
    out = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=out[1:])
    return out, s[order].astype(np.int32), np.ascontiguousarray(b[order]).view(np.float32)
