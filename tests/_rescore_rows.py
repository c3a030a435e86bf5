"""Rows, distance matrices and expected results for the held re-score rows (tests/test_gpu_rescore_rows.py).

The rows are built as tests/test_gpu_sparse_rescore.py builds its fixture: N rows over F = 2^20 ids, the stored-entry
counts at the lane and tile edges first, then short rows from a small sub-pool, with stored zeros, +-0-only rows, empty
rows, duplicates and isolated rows, the values on a coarse grid so that equal distances occur.  The expected result of
a ragged call is taken from the numpy models the sparse searches are held to (tests/_radius_model.py): row q is
D[q, candidates], the entries <= float32(r), sorted by (distance bits, index)."""
import numpy as np

import _radius_model as rmodel
from _weighted_rows import csr as rows_csr
from fedrann_amd import _lib

F = 1 << 20
N = 300
T = _lib.FDR_RESCORE_TILE
METRICS = ("cosine", "jaccard", "weighted_jaccard")
WHICH = METRICS + ("jaccard_sets",)  # "jaccard_sets": Jaccard without values (every stored entry present)
SPECIAL = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)  # row i has SPECIAL[i] stored entries
LONGEST = len(SPECIAL) - 1  # the row of 2 T + 3 stored entries; row 60 is its duplicate
N_ISO = 6  # rows whose ids no other row holds
ZERO_ROWS = (0, 40, 140, 45, 145)  # empty, or +-0 only


def rows(seed=11):
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(F, 2 * T + 1024 + N_ISO, replace=False)).astype(np.int64)
    iso, pool = pool[-N_ISO:], pool[:-N_ISO]
    out = []
    for i in range(N):
        m = SPECIAL[i] if i < len(SPECIAL) else int(rng.integers(1, 41))
        ids = np.sort(rng.choice(pool if m > 40 else pool[:256], m, replace=False))
        vals = (rng.integers(1, 6, size=m) * 0.37).astype(np.float32)
        vals[rng.random(m) < 0.1] = 0.0  # explicit stored zeros
        out.append((ids, vals))
    for i in (40, 140):
        out[i] = (np.zeros(0, np.int64), np.zeros(0, np.float32))  # empty rows
    for i in (45, 145):
        ids = out[i][0]
        out[i] = (ids, np.where(np.arange(ids.size) % 2 == 0, 0.0, -0.0).astype(np.float32))  # only +-0: zero rows
    for i in (50, 150, 250):
        out[i] = out[20]  # duplicates
    out[60] = out[LONGEST]  # a duplicate of the longest row
    for j in range(N_ISO):
        out[70 + 10 * j] = (iso[j:j + 1], np.array([1.5], np.float32))
    return rows_csr(out)


def values_for(metric, values, seed=12):
    """cosine takes signs too; the Jaccard metrics the values as they are"""
    if metric != "cosine":
        return values
    sign = np.where(np.random.default_rng(seed).random(values.size) < 0.3, -1.0, 1.0).astype(np.float32)
    return values * sign


def matrix(metric, oracle, csr, n_features):
    """float32 [n, n]: every row against every row under the models of the searches"""
    if metric == "cosine":
        idx, dist = rmodel.cosine_ranked(oracle, csr, csr)
        D = np.empty(idx.shape, np.float32)
        np.put_along_axis(D, idx.astype(np.int64), dist, axis=1)
        return D
    return rmodel.distances(metric, csr, csr, n_features)


def matrices(csr, oracle):
    """which -> (metric, values, D)"""
    indptr, indices, values = csr
    out = {}
    for metric in METRICS:
        v = values_for(metric, values)
        out[metric] = (metric, v, matrix(metric, oracle, (indptr, indices, v), F))
    out["jaccard_sets"] = ("jaccard", None, matrix("jaccard", oracle, (indptr, indices, None), F))
    return out


def ragged(lists):
    """a list of int arrays -> (cand_indptr int64, cand_idx int32)"""
    ip = np.zeros(len(lists) + 1, np.int64)
    if lists:
        np.cumsum([len(c) for c in lists], out=ip[1:])
    ix = np.concatenate([np.asarray(c, np.int32) for c in lists]) if lists else np.zeros(0, np.int32)
    return ip, np.ascontiguousarray(ix, dtype=np.int32)


def want(D, q_lo, cand_indptr, cand_idx, r):
    """The expected (indptr, idx, dist) of RescoreRows.radius on the queries q_lo .."""
    r = np.float32(r)
    out_ip = np.zeros(cand_indptr.size, np.int64)
    idx, dist = [], []
    for i in range(cand_indptr.size - 1):
        c = cand_idx[cand_indptr[i]:cand_indptr[i + 1]]
        d = D[q_lo + i, c]
        keep = d <= r
        c, d = c[keep], d[keep]
        order = np.lexsort((c, d.view(np.uint32)))  # (last key first: distance bits, then index)
        idx.append(c[order])
        dist.append(d[order])
        out_ip[i + 1] = out_ip[i] + c.size
    return (out_ip, np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32),
            np.concatenate(dist).astype(np.float32) if dist else np.zeros(0, np.float32))


def between(D, lo_frac=0.5):
    """A radius strictly between two distances that occur in D (both below 1), near the lo_frac quantile of the
    distances below 1: (r, the distance below it, the distance above it)"""
    u = np.unique(D[D < 1])
    assert u.size >= 3
    i = min(max(int(u.size * lo_frac), 0), u.size - 2)
    a, b = np.float32(u[i]), np.float32(u[i + 1])
    r = np.float32((np.float64(a) + np.float64(b)) / 2)
    if not a < r < b:  # (neighbouring floats: take the lower one; the bound is closed)
        r = a
    return r, a, b


EDGE_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, N + 40)


def edge_lists(seed=7):
    """One candidate list per query, the lengths cycling over EDGE_LENGTHS (the last: every row and 40 repeats); the
    special rows, the longest row's duplicate and the query itself are written into every non-empty list as far as it
    reaches.  The longest row and its duplicate, as queries, get lists above FDR_MAX_K entries."""
    rng = np.random.default_rng(seed)
    must = list(range(len(SPECIAL))) + [60]
    lists = []
    for q in range(N):
        m = EDGE_LENGTHS[q % len(EDGE_LENGTHS)]
        if q in (LONGEST, 60):
            m = 257 if q == LONGEST else N + 40
        if m <= N:
            c = rng.permutation(N)[:m]
        else:
            c = np.concatenate([rng.permutation(N), rng.integers(0, N, m - N)])
        c = c.astype(np.int32)
        fixed = ([q] + must)[:m]
        c[rng.permutation(m)[:len(fixed)]] = fixed
        lists.append(c)
    return lists
