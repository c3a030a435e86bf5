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

Components (component_labels: the statement fdr_graph_components, csrc/graph_components.inc, is held to).  For a graph
G, a mode m in {union, mutual} and a bound B, the components are the connected components of an undirected graph on the
n rows: rows r != s are joined iff symmetrize_rows(G, m) has the entry (r, s) with distance bits <= bits(B).  B is a
float32 with 0 <= bits(B) <= 0x7f800000; the default, +inf, joins every entry.  Spelled out:

    union      an entry (q -> t) with bits <= bits(B) joins q and t
    mutual     q and t are joined iff each lists the other and min(b(q -> t), b(t -> q)) <= bits(B)

Self entries join nothing; the bound is inclusive and compares bit patterns, so 0.0 and the smallest subnormal are
different distances.  label[r] in [0, C) numbers the components in ascending order of their smallest row, so the labels
are a function of the edge set alone; size[c], int64, is the number of rows of component c.  A graph is refused for
exactly what symmetrize_rows refuses, in both modes and in the same words; transpose is refused as a mode (its
components are union's).

Expansion (expand_rows: the statement fdr_graph_expand, csrc/graph_expand.inc, is held to).  N_f(x) is the first
min(fan, len(x)) entries of row x in ascending order of key = distance bits << 32 | index.  Row r of the result holds s
iff s is in N_f(r), or s != r and s is in N_f(t) for some t in N_f(r): the rows within two hops along the fan, the
row's own index exactly when the row lists itself inside its fan.  Every row is strictly ascending by index and holds
every index once.  Refused, over the whole graph and in the words above: an index outside [0, n); distance bits above
0x7f800000.  An index listed twice in a row is not refused: it takes two places of the fan cut and comes out once.
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


def _entries(indptr, idx, dist):
    """What symmetrize_rows and component_labels share: the rules, then every entry (q -> t) with its reverse.  Returns
    (n, q int64, t int64, bits uint32, has bool: t lists q, low uint32: the smaller bits of the directions present)."""
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
    return n, rows, t, bits, has, low


def symmetrize_rows(indptr, idx, dist, mode):
    """The union / mutual / transposed rows of the ragged graph (indptr, idx, dist), see the module's docstring:
    (indptr int64 [n + 1], idx int32, dist float32), a function of the input alone."""
    code = mode_code(mode)
    n, rows, t, bits, has, low = _entries(indptr, idx, dist)
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


def component_mode_code(mode):
    code = mode_code(mode)
    if code == MODES["transpose"]:
        raise ValueError("mode must be union or mutual for components: those of the transposed rows are the union's")
    return code


def bound_bits(max_distance):
    """The bits of a components bound as float32; None is +inf, which joins every entry.  ValueError unless
    0 <= bits <= 0x7f800000: NaN, negatives and -0.0 are refused."""
    if max_distance is None:
        return MAX_BITS
    if isinstance(max_distance, (bool, np.bool_)) or not isinstance(max_distance, (int, float, np.integer, np.floating)):
        raise ValueError("max_distance must be a number or None, got %r" % (max_distance,))
    with np.errstate(over="ignore"):
        found = int(np.array(max_distance, dtype=np.float64).astype(np.float32).view(np.uint32))
    if found > MAX_BITS:
        raise ValueError("max_distance must be a float32 that is neither negative (-0.0 included) nor NaN: its bits "
                         "must be at most 0x7f800000, got %r" % (max_distance,))
    return found


def component_labels(indptr, idx, dist, mode="union", max_distance=None):
    """The connected components of the ragged graph (indptr, idx, dist) under `mode` ("union" / "mutual"), cut at
    max_distance (None: +inf), see the module's docstring: (labels int32 [n], sizes int64 [C]), components numbered in
    ascending order of their smallest row.  A function of the edge set alone; refuses what symmetrize_rows refuses."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    code = component_mode_code(mode)
    bound = bound_bits(max_distance)
    n, rows, t, bits, has, low = _entries(indptr, idx, dist)
    joined = (rows != t) & ((bits <= bound) if code == MODES["union"] else (has & (low <= bound)))
    links = coo_matrix((np.ones(int(joined.sum()), np.int8), (rows[joined], t[joined])), shape=(n, n))
    _, found = connected_components(links, directed=False)
    _, first = np.unique(found, return_index=True)  # every component's smallest row
    number = np.empty(first.size, np.int32)
    number[np.argsort(first)] = np.arange(first.size, dtype=np.int32)
    labels = number[found]
    return labels, np.bincount(labels, minlength=first.size).astype(np.int64)


FDR_MAX_K = 128  # include/fedrann_hip.h


def check_expand(indptr, idx, dist, fan, lo=0, hi=None):
    """The argument checks expand_rows and _lib.check_graph_expand share (ValueError): the ragged graph, at least one
    row, 1 <= fan <= FDR_MAX_K, [lo, hi) a range of the rows (hi None: n).  Returns (indptr, idx, dist, n, fan, lo, hi)."""
    indptr, idx, dist = as_ragged((indptr, idx, dist))
    n = indptr.size - 1
    if n < 1:
        raise ValueError("a graph has at least one row")
    for name, v in (("fan", fan), ("lo", lo)) + ((("hi", hi),) if hi is not None else ()):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    fan, lo, hi = int(fan), int(lo), n if hi is None else int(hi)
    if not 1 <= fan <= FDR_MAX_K:
        raise ValueError("need 1 <= fan <= %d, got %d" % (FDR_MAX_K, fan))
    if not 0 <= lo <= hi <= n:
        raise ValueError("the rows [%d, %d) are no range of the n = %d rows" % (lo, hi, n))
    return indptr, idx, dist, n, fan, lo, hi


def expand_bound(indptr, fan):
    """int64 [n]: fan-cut length times (1 + fan), an upper bound of what row r gathers before duplicates go that needs
    the row pointer alone (the exact bound, |N_f(r)| + the sum of |N_f(t)| over t in N_f(r), needs the sorted rows)."""
    return np.minimum(np.diff(np.asarray(indptr, np.int64)), int(fan)) * (1 + int(fan))


def expand_rows(indptr, idx, dist, fan, lo=0, hi=None, piece_entries=1 << 24):
    """The rows within two hops of the rows [lo, hi) of the ragged graph (indptr, idx, dist) along a fan of `fan`, see
    the module's docstring: (indptr int64 [hi - lo + 1], idx int32), every row ascending by index, a function of the
    input alone.  The whole graph is checked, whatever the range.  The rows are walked in pieces whose gathered entries
    stay near piece_entries."""
    indptr, idx, dist, n, fan, lo, hi = check_expand(indptr, idx, dist, fan, lo, hi)
    lens = np.diff(indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    t = idx.astype(np.int64)
    bits = dist.view(np.uint32)
    records = np.concatenate([rows[(t < 0) | (t >= n)] * 4, rows[bits > MAX_BITS] * 4 + 1])
    if records.size:
        worst = int(records.min())
        raise ValueError("row %d: %s" % (worst // 4, RULES[worst % 4]))
    # ---- the fan cut: every row by key, its first `fan` entries ----
    order = np.lexsort((t, bits, rows))
    keep = (np.arange(t.size, dtype=np.int64) - indptr[rows]) < fan  # (rows[order] == rows: the sort keeps the segments)
    ft = t[order][keep]
    flen = np.minimum(lens, fan)
    fptr = np.zeros(n + 1, np.int64)
    np.cumsum(flen, out=fptr[1:])
    counts = np.zeros(hi - lo, np.int64)
    parts = []
    bound = expand_bound(indptr, fan)[lo:hi]
    a = lo
    while a < hi:
        b = a + max(1, int(np.searchsorted(np.cumsum(bound[a - lo:]), piece_entries, side="right")))
        b = min(b, hi)
        one_r = np.repeat(np.arange(a, b, dtype=np.int64), flen[a:b])
        one_t = ft[fptr[a]:fptr[b]]
        reps = flen[one_t]
        two_r = np.repeat(one_r, reps)
        first = np.repeat(fptr[one_t] - (np.cumsum(reps) - reps), reps)  # N_f(t)'s start less the entry's place
        two_s = ft[first + np.arange(two_r.size, dtype=np.int64)]
        far = two_s != two_r
        code = np.unique(np.concatenate([one_r * n + one_t, two_r[far] * n + two_s[far]]))
        counts[a - lo:b - lo] = np.bincount(code // n - a, minlength=b - a)
        parts.append((code % n).astype(np.int32))
        a = b
    out = np.zeros(hi - lo + 1, np.int64)
    np.cumsum(counts, out=out[1:])
    return out, np.concatenate(parts) if parts else np.zeros(0, np.int32)
