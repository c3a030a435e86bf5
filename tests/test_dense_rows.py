"""The dense row generators of tests/_dense_rows.py can see a change of summation order (CPU only).

A kernel that sums a dot product in another order -- a split-K chain whose second half starts from +0 and is added at
the end, a hand-off one chunk off -- changes the distance bits of only those pairs whose fp32 result depends on the
order.  For the GPU tests on these rows to catch such a kernel, a large share of the pairs the k-NN ranks must be such
pairs.  Measured with the oracle's own pair distance: the components summed ascending, rotated by 512 and reversed."""
import numpy as np
import pytest

import _dense_rows as D
from test_gpu_wide_knn import _rows

MIN_SHARE = 0.25


def _near_pairs(oracle, E, seed, nq=40, k=50, per=10):
    """(query, target) pairs from the queries' k nearest rows: the pairs whose bits decide a k-NN result."""
    rng = np.random.default_rng(seed)
    Eh, _, zero = oracle.normalize(E)
    q = rng.choice(np.flatnonzero(zero == 0), size=nq, replace=False)
    idx, _ = oracle.knn_normalized(Eh[q], zero[q], Eh, zero, k)
    return [(a, b) for a, row in zip(q, idx) for b in rng.choice(row[1:], size=per, replace=False)]


def _orders(d):
    return {"rotated by 512": np.roll(np.arange(d), 512), "reversed": np.arange(d)[::-1]}


@pytest.mark.parametrize("kind", D.GENERATORS)
@pytest.mark.parametrize("d", [1000, 2048])
def test_dense_generators_see_the_summation_order(oracle, kind, d):
    E = D.make(kind, 2000, d, 3)
    assert np.any(~E.any(axis=1))  # (zero rows mixed in)
    pairs = _near_pairs(oracle, E, d)
    for name, perm in _orders(d).items():
        share = D.order_sensitivity(oracle, E, pairs, perm)
        assert share >= MIN_SHARE, (kind, d, name, share)


def test_mixed_set_sees_the_summation_order(oracle):
    E, _ = D.mixed(3000, 1000, 9)
    pairs = _near_pairs(oracle, E, 9)
    for name, perm in _orders(1000).items():
        assert D.order_sensitivity(oracle, E, pairs, perm) >= MIN_SHARE, name


def test_sparse_rows_of_the_older_tests_do_not(oracle):
    """Documentation: the six-non-zero rows of tests/test_gpu_wide_knn.py fail the same check (about 0.04 % of pairs
    change), which is why the dense rows exist."""
    E = _rows(3000, 1000, 1)
    pairs = _near_pairs(oracle, E, 1)
    for name, perm in _orders(1000).items():
        assert D.order_sensitivity(oracle, E, pairs, perm) < 0.01, name


def test_halves_at_513_isolate_the_last_component():
    E = D.halves(2000, 513, 4)
    single = np.flatnonzero((E[:, 512] != 0) & ~E[:, :512].any(axis=1))
    assert single.size >= 2
    lo = E[:, :512].any(axis=1) & ~E[:, 512:].any(axis=1)
    hi = ~E[:, :448].any(axis=1) & E[:, 512:].any(axis=1)
    assert lo.sum() > 100 and hi.sum() > 100


def test_clusters_hold_near_ties_and_far_duplicates():
    n = 2000
    E = D.clusters(n, 1000, 6)
    dup = [i for i in range(n // 2) if E[i].any() and np.array_equal(E[i], E[i + n // 2])]
    assert len(dup) >= 8


def test_sample_rows_cover_block_edges():
    rows = D.sample_rows(9001, 1)
    assert {0, 9000}.issubset(rows) and rows.min() >= 0 and rows.max() < 9001
    for m in (32, 64, 128):
        assert np.any(rows % m == 0) and np.any(rows % m == m - 1)
