"""Neighbour graphs for the symmetrise tests (host and GPU), and a brute force of the definition that shares nothing
with fedrann_amd.graph: a dict of pairs and Python's own sort.

Graphs are ragged (indptr int64 [n + 1], idx int32, dist float32).  Row lengths come from {0, 0, 1, 63, 64, 65, 300}
capped at n, a row's indices are distinct, and distances come from {0, 0.25, 0.5} only, so the index decides most
positions of a result row."""
import numpy as np

LENGTHS = (0, 0, 1, 63, 64, 65, 300)
LEVELS = (0.0, 0.25, 0.5)
MODES = ("union", "mutual", "transpose")


def from_rows(rows):
    """[[(index, distance), ...], ...] -> the ragged triple."""
    ip = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ip[1:])
    flat = [e for r in rows for e in r]
    return ip, np.array([e[0] for e in flat], np.int32), np.array([e[1] for e in flat], np.float32)


def bits(dist):
    return np.ascontiguousarray(dist, dtype=np.float32).view(np.uint32)


def sort_rows(graph):
    """every row by (distance bits, index)"""
    ip, idx, dist = graph
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    order = np.lexsort((idx, bits(dist), rows))
    return ip, idx[order], dist[order]


def drawn(n, seed, shuffled=False, levels=LEVELS, lengths=LENGTHS):
    """A random graph on n rows; rows sorted by key, or in the order drawn (shuffled)."""
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.choice(np.asarray(lengths), size=n), n)
    ip = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=ip[1:])
    idx = np.concatenate([rng.permutation(n)[:m] for m in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    dist = rng.choice(np.asarray(levels, np.float32), size=idx.size).astype(np.float32)
    return (ip, idx, dist) if shuffled else sort_rows((ip, idx, dist))


def brute(graph, mode):
    """The definition, pair by pair."""
    ip, idx, dist = graph
    n = ip.size - 1
    b = bits(dist)
    listed = {}
    for q in range(n):
        for e in range(int(ip[q]), int(ip[q + 1])):
            listed[(q, int(idx[e]))] = int(b[e])
    rows = [[] for _ in range(n)]
    if mode == "transpose":
        for (q, t), v in listed.items():
            rows[t].append((v, q))
    else:
        for (q, t), v in listed.items():
            back = listed.get((t, q))
            if back is not None:
                rows[q].append((min(v, back), t))
            elif mode == "union":
                rows[q].append((v, t))
                rows[t].append((v, q))
    out = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=out[1:])
    flat = [e for r in rows for e in sorted(r)]
    return (out, np.array([e[1] for e in flat], np.int32),
            np.array([e[0] for e in flat], np.uint32).view(np.float32))


def pairs(graph):
    """{(row, index)}"""
    ip, idx, _ = graph
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return set(zip(rows.tolist(), idx.tolist()))


TINY = float(np.array([1], np.uint32).view(np.float32)[0])  # the smallest subnormal


def asymmetric():
    """5 rows whose two directions disagree in bits, 0.0 against the smallest subnormal included, with self entries
    (row 2's at a non-zero distance) and a one-way pair."""
    return from_rows([
        [(1, 0.5), (0, 0.0), (3, TINY)],   # 0 -> 1 at 0.5 (1 -> 0 at 0.25); 0 -> 3 at the subnormal (3 -> 0 at 0.0)
        [(0, 0.25), (2, 0.75)],            # 1 -> 2 at 0.75 (2 -> 1 at 0.125)
        [(2, 0.375), (1, 0.125), (4, 0.5)],  # 2 -> 4 one way
        [(0, 0.0)],
        [],
    ])
