"""Sparse rows with non-negative values for the weighted Jaccard tests (host and GPU): the constructions of the Jaccard
tests, with positive values on a coarse grid so that equal masses and equal minima occur."""
import numpy as np


def csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([r[0].size for r in rows])
    indices = np.concatenate([r[0] for r in rows]).astype(np.int32)
    values = np.concatenate([r[1] for r in rows]).astype(np.float32)
    return indptr, indices, values


def weighted_rows(n, seed, F=1 << 25, n_ids=512, per=(1, 12), zeros=0.1):
    """CSR rows over feature ids spread across [0, F) but drawn from n_ids distinct ids, values in {1..5} * 0.37:
    about 10 % explicit stored zeros, empty rows, rows of +-0 only, exact duplicates, rows with equal supports under
    different values, and isolated rows (ids no other row holds).  Returns (indptr, indices, values)."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(F, n_ids, replace=False)).astype(np.int64)
    n_iso = min(64, n_ids // 4)
    iso = pool[-n_iso:]  # the isolated rows' private ids
    rows = []
    for i in range(n):
        m = int(rng.integers(per[0], per[1] + 1))
        ids = np.sort(rng.choice(pool[:-n_iso], m, replace=False))
        vals = (rng.integers(1, 6, size=m) * 0.37).astype(np.float32)
        vals[rng.random(m) < zeros] = 0.0  # explicit stored zeros: absent entries
        rows.append((ids, vals))
    for i in range(0, n, 97):
        rows[i] = (np.zeros(0, np.int64), np.zeros(0, np.float32))  # empty row
    for i in range(5, n, 131):
        ids = rows[i][0]
        rows[i] = (ids, np.where(np.arange(ids.size) % 2 == 0, 0.0, -0.0).astype(np.float32))  # only +-0: zero mass
    if n > 4:
        for i in range(7, n, 53):
            rows[i] = rows[3]  # duplicates
        for i in range(11, n, 71):
            ids, vals = rows[4]
            rows[i] = (ids, np.where(vals != 0, np.float32(9.5), np.float32(0)).astype(np.float32))  # equal supports
    for j, i in enumerate(range(13, n, max(1, n // 64))):
        if j < iso.size:
            rows[i] = (iso[j:j + 1], np.array([1.5], np.float32))  # isolated: alone with its id
    return csr(rows)
