"""Graphs for the components tests (host and GPU), and a brute force of the definition that shares nothing with
fedrann_amd.graph: the pairs of _graph_rows.brute(graph, mode), filtered by their bits, through a dict union-find.

The union graphs are _graph_rows.drawn with short rows (lengths 0, 0, 1, 1, 2): near the threshold at which a random
graph grows its giant component, so a draw on 1000 rows has one large component, tens of middling ones and hundreds of
single rows.  The mutual graphs start from rows of 0, 1, 1, 2, 3 entries and reciprocate 60 % of them: a plain draw
has hardly a reciprocated pair, and every mutual component of it is a single row."""
import numpy as np

import _graph_rows as gr

UNION_LENGTHS = (0, 0, 1, 1, 2)
MUTUAL_LENGTHS = (0, 1, 1, 2, 3)
BOUNDS = (None, 0.25, 0.0)
COMPONENT_MODES = ("union", "mutual")


def shuffle_rows(graph, seed):
    """every row's entries in a random order"""
    ip, idx, dist = graph
    rng = np.random.default_rng(seed)
    order = np.concatenate([int(ip[r]) + rng.permutation(int(ip[r + 1] - ip[r])) for r in range(ip.size - 1)]
                           + [np.zeros(0, np.int64)]).astype(np.int64)
    return ip, idx[order], dist[order]


def reciprocated(n, seed, shuffled=False):
    """drawn(n, seed, lengths=MUTUAL_LENGTHS) in which, for each entry (q -> t), with probability 0.6 the reverse
    (t -> q) is added at a level of its own, unless t lists q already."""
    ip, idx, dist = gr.drawn(n, seed, lengths=MUTUAL_LENGTHS)
    rng = np.random.default_rng(seed + 1000)
    coin = rng.random(idx.size) < 0.6
    level = rng.choice(np.asarray(gr.LEVELS, np.float32), size=idx.size)
    rows = [[(int(idx[e]), float(dist[e])) for e in range(int(ip[q]), int(ip[q + 1]))] for q in range(n)]
    listed = {(q, t) for q in range(n) for t, _ in rows[q]}
    for q in range(n):
        for e in range(int(ip[q]), int(ip[q + 1])):
            t = int(idx[e])
            if coin[e] and (t, q) not in listed:
                listed.add((t, q))
                rows[t].append((q, float(level[e])))
    graph = gr.from_rows(rows)
    return shuffle_rows(graph, seed + 2000) if shuffled else gr.sort_rows(graph)


def graph_for(mode, n, seed, shuffled=False):
    """the test graph of a mode: short drawn rows (union), reciprocated rows (mutual)"""
    if mode == "mutual":
        return reciprocated(n, seed, shuffled)
    return gr.drawn(n, seed, shuffled=shuffled, lengths=UNION_LENGTHS)


def bound_bits(bound):
    return 0x7f800000 if bound is None else int(gr.bits(np.float32(bound).reshape(1))[0])


def joined_pairs(graph, mode, bound=None):
    """[(r, s)], r != s: the entries of the brute-force symmetrised rows with bits <= bits(bound)"""
    ip, idx, dist = gr.brute(graph, mode)
    top = bound_bits(bound)
    b = gr.bits(dist)
    out = []
    for r in range(ip.size - 1):
        for e in range(int(ip[r]), int(ip[r + 1])):
            if int(idx[e]) != r and int(b[e]) <= top:
                out.append((r, int(idx[e])))
    return out


def by_smallest_row(names):
    """any naming of the rows' components -> (labels int32, sizes int64), numbered by their smallest row"""
    number = {}
    labels = np.empty(len(names), np.int32)
    for r, name in enumerate(names):
        labels[r] = number.setdefault(name, len(number))
    return labels, np.bincount(labels, minlength=len(number)).astype(np.int64)


def brute_components(graph, mode, bound=None):
    """The definition: a dict union-find over the joined pairs."""
    n = graph[0].size - 1
    parent = {r: r for r in range(n)}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for r, s in joined_pairs(graph, mode, bound):
        a, b = find(r), find(s)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return by_smallest_row([find(r) for r in range(n)])


def profile(sizes):
    """(C, the largest, the singletons, the components of 3 - 49 rows)"""
    sizes = np.asarray(sizes)
    return int(sizes.size), int(sizes.max()), int(np.sum(sizes == 1)), int(np.sum((sizes >= 3) & (sizes <= 49)))


def is_rich(sizes):
    """what a test graph on 1000 rows must offer: middling components, a large one and single rows"""
    _, largest, singles, middling = profile(sizes)
    return middling >= 10 and largest >= 50 and singles >= 100


def equal(got, want):
    """labels and sizes, array for array, dtypes included"""
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (got[1].shape, want[1].shape)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
