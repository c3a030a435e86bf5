"""Radius search on the dense index in numpy: what fdr_dense_index_radius_search / _radius_query must give, bit for
bit, and the fp16 view of the same pairs that the range pass takes.

The exact result comes from the oracle alone: oracle.knn_normalized at k = n ranks ALL targets of every query in
(distance bits, index) order with the canonical chain, and _radius_model.cut_ranked keeps each row's prefix with
distance <= r.  Nothing here knows the kernels.

The fp16 view: approx_dists() rounds both sides with _candidate_model.to_half and accumulates in float32, the
quantity d~ the range pass compares with th = r + MARGIN.  worst_pair() finds the pair with distance < 1 whose d~
exceeds its canonical distance the most: at a radius equal to that pair's distance the pair is a hit with d~ > r, which
a pass without the margin would drop.
"""
import numpy as np

import _candidate_model as cmodel
import _dense_rows
import _radius_model as rmodel
from test_gpu_parity import _adversarial_rows

# radius_margin() of knn_plan.inc, in the same fp32 arithmetic
MARGIN = np.float32(np.float32(cmodel.PREFILTER_EPS) + np.float32(1.0e-6))

ADVERSARIAL = tuple((kind, d) for kind in ("fp16_midpoints", "fp16_subnormals", "dense") for d in (128, 256, 500))
N_ADVERSARIAL = 1000


def adversarial(kind, d, n=N_ADVERSARIAL):
    """The set (kind, d) of the tests, always the same rows."""
    return _adversarial_rows(kind, n, d, np.random.default_rng(1000 * d + len(kind)))


def mixed(n=999, d=100, seed=7):
    return _dense_rows.mixed(n, d, seed)[0]


def ranked(oracle, E, Q=None):
    """(idx, dist) [nq, n]: all n rows of E for every row of Q (None: E itself), in (distance bits, index) order."""
    Eh, _, ez = oracle.normalize(E)
    if Q is None:
        Qh, qz = Eh, ez
    else:
        Qh, _, qz = oracle.normalize(Q)
    return oracle.knn_normalized(Qh, qz, Eh, ez, E.shape[0])


def model(oracle, E, Q=None, lo=0, hi=None):
    """r -> the ragged result of the queries [lo, hi); the oracle's ranking is computed once."""
    idx, dist = ranked(oracle, E, Q)
    idx, dist = idx[lo:hi], dist[lo:hi]
    return lambda r: rmodel.cut_ranked(idx, dist, r)


def exact_dists(oracle, E):
    """The canonical float32 distance of every pair, [n, n], from the ranking."""
    idx, dist = ranked(oracle, E)
    D = np.empty_like(dist)
    np.put_along_axis(D, idx.astype(np.int64), dist, axis=1)
    return D


def approx_dists(oracle, E):
    """d~ [n, n]: fp16 operands (round to nearest even), float32 accumulation, clamp(1 - s~, 0, 1) in float32."""
    Eh, _, _ = oracle.normalize(E)
    h = cmodel.to_half(Eh)
    s = (h @ h.T).astype(np.float32)
    return np.clip(np.float32(1.0) - s, np.float32(0.0), np.float32(1.0)).astype(np.float32)


def scanned(oracle, E):
    """bool [n]: the queries that take part in the fp16 scan, the non-zero rows (a zero query's row is the closed form:
    the zero rows at distance 0, which the fp16 view puts at 1)."""
    return oracle.normalize(E)[2] == 0


def worst_pair(D, Dt):
    """(q, t, distance): the pair with canonical distance in (0, 1) whose fp16 distance lies furthest ABOVE it."""
    gap = np.where((D > 0.0) & (D < 1.0), Dt.astype(np.float64) - D.astype(np.float64), -np.inf)
    q, t = np.unravel_index(int(np.argmax(gap)), gap.shape)
    return int(q), int(t), np.float32(D[q, t])


def radii(D, Dt):
    """The radii of a set, all taken from the oracle's own distances: 0; the worst pair's distance (an inclusive
    boundary where the margin is needed) and the float32 just below it; the distance of the sixth neighbour of the
    middle row; the largest distance below 1."""
    n = D.shape[0]
    rb = worst_pair(D, Dt)[2]
    below1 = D[D < 1.0]
    out = [np.float32(0.0), rb, np.nextafter(rb, np.float32(0.0)), np.sort(D[n // 2])[min(5, n - 1)]]
    if below1.size:
        out.append(below1.max())
    return [np.float32(r) for r in out if 0.0 <= r < 1.0]
