"""A model of the duplicate-row class layer (fedrann_amd/csrc/dedup_classes.inc) in plain numpy, for the tests that
drive expand_classes_kernel with lists of their own (tests/test_gpu_class_expand.py) and for the CPU test that shows the
model itself right against the oracle (tests/test_class_model.py).  It shares nothing with the kernel: classes come
from a dictionary of the rows' bytes, the expansion from a sort of (distance bits, row) pairs.

Numbering.  A class is named by its UNIQUE-ROW number: classes in ascending order of their smallest member (their
representative), the order in which the library stores the unique rows.  So `cls_of_row` is also `u_of_row`, and
members[u][0] is unique row u's representative."""
import numpy as np

STRATA = ("fast", "concat", "sort32", "sort64", "sort128", "select")
TIE_STRATA = STRATA[2:]


def classes_of(T):
    """T: the (padded) rows, float32 [n, dp].  Rows are one class when all their 32-bit words are equal (-0.0 and +0.0
    differ).  Returns (cls_of_row int64 [n], members, reps): members[u] the rows of class u ascending (int64), reps[u] =
    members[u][0] ascending in u."""
    T = np.ascontiguousarray(T, dtype=np.float32)
    words = T.view(np.uint32)
    first, rows = {}, []
    cls_of_row = np.empty(T.shape[0], dtype=np.int64)
    for r in range(T.shape[0]):  # (ascending r: a class is numbered when its smallest member turns up)
        u = first.setdefault(words[r].tobytes(), len(rows))
        if u == len(rows):
            rows.append([])
        rows[u].append(r)
        cls_of_row[r] = u
    members = [np.asarray(m, dtype=np.int64) for m in rows]
    return cls_of_row, members, np.asarray([m[0] for m in members], dtype=np.int64)


def _bits(dist_u):
    a = np.ascontiguousarray(dist_u)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.uint32)


def expand_one(members, ids, bits, k, t_base=0):
    """One unique row's list (k unique-row ids, k distance bit patterns) -> the k smallest (bits, row) over the first k
    members of every listed class: (rows + t_base as int32 [k], bits uint32 [k])."""
    pairs = []
    for u, b in zip(ids, bits):
        pairs += [(int(b), int(m)) for m in members[int(u)][:k]]
    pairs.sort()
    assert len(pairs) >= k
    pairs = pairs[:k]
    return (np.asarray([t_base + m for _, m in pairs], dtype=np.int64).astype(np.int32),
            np.asarray([b for b, _ in pairs], dtype=np.uint32))


def expand(members, u_of_row, idx_u, dist_u, q0, nq, k, t_base):
    """The lists of rows [q0, q0 + nq): row i takes the list of its unique row u_of_row[i] (idx_u / dist_u: [nu, k],
    dist_u float32 or its bits).  Returns (idx int32 [nq, k], distance bits uint32 [nq, k])."""
    bits_u = _bits(dist_u)
    idx = np.empty((nq, k), dtype=np.int32)
    bits = np.empty((nq, k), dtype=np.uint32)
    done = {}
    for i in range(nq):
        u = int(u_of_row[q0 + i])
        if u not in done:  # (a row's answer is a function of its class alone)
            done[u] = expand_one(members, idx_u[u, :k], bits_u[u, :k], k, t_base)
        idx[i], bits[i] = done[u]
    return idx, bits


def path_one(sizes, bits, k):
    """The way expand_classes_kernel takes for one list, by the kernel's own definition: sizes[r] the size of slot r's
    class, bits[r] its distance bits."""
    sizes = [int(s) for s in sizes[:k]]
    assert len(sizes) == k
    if all(s == 1 for s in sizes):
        return "fast"
    m = [min(k, s) for s in sizes]
    base = [sum(m[:r]) for r in range(k)]
    n = sum(m)
    tie = any(r + 1 < k and base[r] < k and int(bits[r]) == int(bits[r + 1]) for r in range(k))
    if not tie:
        return "concat"
    return "sort32" if n <= 32 else "sort64" if n <= 64 else "sort128" if n <= 128 else "select"


def path_of(members, idx_u, dist_u, k, u_of_row=None, q0=0, nq=None):
    """path_one for every list of idx_u / dist_u ([nu, k]): an array of names, one per unique row; with u_of_row, one
    per query row of [q0, q0 + nq)."""
    bits_u = _bits(dist_u)
    size = np.asarray([len(m) for m in members], dtype=np.int64)
    per_u = np.asarray([path_one(size[np.asarray(idx_u[u, :k], dtype=np.int64)], bits_u[u, :k], k)
                        for u in range(idx_u.shape[0])], dtype=object)
    if u_of_row is None:
        return per_u
    nq = len(u_of_row) - q0 if nq is None else nq
    return per_u[np.asarray(u_of_row[q0:q0 + nq], dtype=np.int64)]


def reachable(k):
    """The strata some list of k slots can land in, from the definitions alone.  A class contributes min(k, size)
    elements, so a list with a class of several rows has n from k + 1 (k >= 2: one class of two) to k * k; k = 1 has
    n = 1 whatever the class and no pair of slots to tie."""
    out = ["fast", "concat"]
    if k >= 2:
        lo, hi = k + 1, k * k  # the n of a list that is not `fast`
        for name, a, b in (("sort32", lo, 32), ("sort64", 33, 64), ("sort128", 65, 128), ("select", 129, hi)):
            if max(a, lo) <= min(b, hi):
                out.append(name)
    return tuple(out)


def counts(paths):
    return {s: int(np.sum(paths == s)) for s in STRATA}


def hot_rows(n, d, seed):
    """n sparse rows with duplicates, shuffled (float32 [n, d], d a multiple of 4), made so that real k-NN lists over
    their unique rows fall into every kind of stratum:
      - all-zero rows (one class, 0 from each other and 1 from everything else);
      - one-hot rows s * (+-e_a) on the first d / 2 components, s in {1, 2, 0.5, 3}: after normalisation at most d
        classes of very different sizes, every two of them at distance exactly 1 (orthogonal, or opposite and clamped);
      - two-hot rows s * (+-e_a +- e_b) on the same components, one to three copies each: many small classes on the
        plateaus 1 - 1/sqrt(2), 1/2 and 1;
      - a cluster of distinct dense rows on the third quarter of the components: lists of one-member classes;
      - a cluster of dense rows on the last quarter, each one to three times: classes of several rows at distinct
        distances."""
    rng = np.random.default_rng(seed)
    h, q = d // 2, d // 4
    n_zero, n_a, n_b = max(2, n // 40), n // 8, n // 6
    n_two = (n - n_zero - n_a - n_b) * 2 // 5
    n_one = n - n_zero - n_a - n_b - n_two
    scale = np.array([1.0, 2.0, 0.5, 3.0], dtype=np.float32)
    rows = [np.zeros((n_zero, d), dtype=np.float32)]
    # one-hot: class (a, sign) drawn with weight ~ 1 / rank^1.5, so a few classes hold most rows and some hold one
    w = 1.0 / np.arange(1, 2 * h + 1) ** 1.5
    cls = rng.permutation(2 * h)[rng.choice(2 * h, n_one, p=w / w.sum())]
    one = np.zeros((n_one, d), dtype=np.float32)
    one[np.arange(n_one), cls // 2] = (1 - 2 * (cls % 2)) * scale[rng.integers(0, 4, n_one)]
    rows.append(one)
    two = np.zeros((n_two, d), dtype=np.float32)
    t = 0
    while t < n_two:
        a, b = rng.choice(h, 2, replace=False)
        sa, sb = rng.choice((-1.0, 1.0), 2)
        for _ in range(min(int(rng.integers(1, 4)), n_two - t)):
            s = scale[rng.integers(0, 3)]  # (a power of two: the normalised copies are bit-equal)
            two[t, a], two[t, b] = sa * s, sb * s
            t += 1
    rows.append(two)
    for lo, cnt, copies in ((h, n_a, 1), (h + q, n_b, 3)):
        centre = rng.standard_normal(q).astype(np.float32)
        blk = np.zeros((cnt, d), dtype=np.float32)
        t = 0
        while t < cnt:
            v = centre + np.float32(0.4) * rng.standard_normal(q).astype(np.float32)
            for _ in range(min(int(rng.integers(1, copies + 1)), cnt - t)):
                blk[t, lo:lo + q] = v
                t += 1
        rows.append(blk)
    E = np.concatenate(rows)
    assert E.shape == (n, d)
    return np.ascontiguousarray(E[rng.permutation(n)])
