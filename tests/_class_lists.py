"""Made-up targets and made-up unique-row lists for tests/test_gpu_class_expand.py: rows whose duplicate-row classes
have chosen sizes, and per unique row a list of k unique-row ids with distance bits built for one stratum of
expand_classes_kernel (tests/_class_model.py names the strata).  Plain numpy, no device: tests/test_class_model.py checks
on the CPU that the seeds used on the GPU meet the floor per stratum."""
import numpy as np

import _class_model as M

N, D = 3000, 8
KS = (1, 2, 3, 7, 20, 21, 22, 32, 33, 45, 46, 63, 64)
FLOOR = 8  # lists (each the list of at least one query) per reachable stratum; mixed ballots and waves
# distance bit patterns: 0.0, the smallest subnormal, 0.5 and its successor (one bit apart), 1.0, 2.0
SPECIAL = np.array([0x00000000, 0x00000001, 0x3F000000, 0x3F000001, 0x3F800000, 0x40000000], dtype=np.uint32)
assert SPECIAL.view(np.float32).tolist() == [0.0, 2.0 ** -149, 0.5, 0.5 + 2.0 ** -24, 1.0, 2.0]


# ---- the targets ---------------------------------------------------------------------------------------------------
def _class_sizes(rng, k, n):
    """One class of 700, two of 200, three each of k - 1, k, k + 1, the rest drawn from {1, 1, 1, 2, 3} until n rows."""
    sizes = [700, 200, 200] + [s for s in (k - 1, k, k + 1) if s >= 1] * 3
    left = n - sum(sizes)
    assert left > n // 3
    while left:
        s = min(int(rng.choice((1, 1, 1, 2, 3))), left)
        sizes.append(s)
        left -= s
    return sizes


def target_rows(k, dp, seed):
    """N rows at D = 8 padded to dp: class c is the small-integer vector (1, digits of c + 1 in base 5); the last two
    rows' classes share their digits and differ in component 0 alone, +0.0 against -0.0.  The members of every class
    are scattered over the whole index range by one permutation."""
    rng = np.random.default_rng(seed)
    sizes = _class_sizes(rng, k, N - 2)
    label = np.concatenate([np.repeat(np.arange(len(sizes)), sizes), [len(sizes), len(sizes)]])
    vec = np.zeros((N, dp), dtype=np.float32)
    vec[:, 0] = 1.0
    c = label + 1
    for j in range(1, D):
        vec[:, j] = c % 5
        c = c // 5
    assert np.all(c == 0)
    vec[N - 2, 0], vec[N - 1, 0] = 0.0, -0.0
    T = np.empty_like(vec)
    T[rng.permutation(N)] = vec
    return T


# ---- the lists -----------------------------------------------------------------------------------------------------
class _Pools:
    def __init__(self, members, k):
        size = np.array([len(m) for m in members])
        self.size, self.k = size, k
        self.m = np.minimum(size, k)
        self.single = np.flatnonzero(size == 1)
        self.multi = np.flatnonzero(size > 1)
        self.full = np.flatnonzero(size >= k) if k > 1 else self.multi  # classes that fill a list by themselves
        self.max_n = int(np.sort(self.m)[::-1][:k].sum())
        assert self.single.size >= 2 * k and self.full.size >= 3


def _levels(rng, cnt):
    """cnt distinct bit patterns, ascending: drawn from SPECIAL while it lasts, then further positive floats below 2.0"""
    if cnt <= SPECIAL.size:
        return np.sort(rng.permutation(SPECIAL)[:cnt])
    more = set()
    while len(more) < cnt - SPECIAL.size:
        more.add(int(rng.integers(2, 0x40000000)))
        more -= set(SPECIAL.tolist())
    return np.sort(np.concatenate([SPECIAL, np.array(sorted(more), dtype=np.uint32)]))


def _sorted(ids, bits):
    ids, bits = np.asarray(ids, dtype=np.int64), np.asarray(bits, dtype=np.uint32)
    assert len(set(ids.tolist())) == ids.size
    order = np.lexsort((ids, bits))  # the kernel's precondition: ascending (bits, unique id)
    return ids[order], bits[order]


def _gen_fast(rng, P):
    ids = rng.choice(P.single, P.k, replace=False)
    if rng.random() < 0.5:  # plateaus: nothing to resolve among one-member classes
        return _sorted(ids, rng.choice(_levels(rng, 3), P.k))
    return _sorted(ids, _levels(rng, P.k))


def _gen_concat(rng, P):
    """classes of several rows at strictly increasing distances; one slot in two holds the cut in a class that fills
    a list by itself"""
    k = P.k
    n_multi = int(rng.integers(1, max(2, k // 2 + 1)))
    ids = list(rng.choice(P.multi, min(n_multi, k), replace=False))
    if rng.random() < 0.5 and not set(ids) & set(P.full.tolist()):
        ids[0] = int(rng.choice(P.full))
    ids += list(rng.choice(P.single, k - len(ids), replace=False))
    return np.asarray(rng.permutation(ids), dtype=np.int64), _levels(rng, k)  # (bits ascending: any slot order will do)


def _gen_tie(lo, hi):
    """bits from three levels (or two, or one), classes chosen so that n = sum of min(k, size) lands in (lo, hi]"""
    def gen(rng, P):
        k = P.k
        a, b = max(lo + 1, k + 1), min(hi, P.max_n)
        if k < 2 or a > b:
            return None
        extra = P.m - 1  # what a class adds to n when it takes a one-member class's slot
        for _ in range(8):
            left, ids = int(rng.integers(a, b + 1)) - k, []
            while left > 0 and len(ids) < k:
                ok = (extra >= 1) & (extra <= left)
                ok[ids] = False
                need = -(-left // (k - len(ids)))  # per slot still free, if every one of them is to help
                if need > 2:  # (small classes alone no longer get there)
                    ok &= extra >= min(need, int(extra[ok].max(initial=0)))
                if not ok.any():
                    break
                ids.append(int(rng.choice(np.flatnonzero(ok))))
                left -= int(extra[ids[-1]])
            n = k + int(extra[ids].sum())
            if lo < n <= hi and ids:
                break
        else:
            return None
        ids += list(rng.choice(P.single, k - len(ids), replace=False))
        lv = SPECIAL[2:5] if rng.random() < 0.3 else _levels(rng, 3)  # (0.5, its successor, 1.0: one bit decides)
        # one list in two uses fewer levels: on ONE plateau the answer is the k smallest rows of all n elements, so
        # every element counts, the last of a long list too
        lv = lv[:int(rng.choice((1, 2, 3, 3)))]
        return _sorted(rng.permutation(ids), rng.choice(lv, k))
    return gen


def _gen_tie_behind(rng, P):
    """a plateau that begins behind the first k elements (base_r >= k): stays a concatenation.  Either slot 0 fills the
    list, or slot 0 has one row and slot 1 a class of k - 1 or more."""
    k = P.k
    if k < 3:
        return None
    lv = _levels(rng, 3)
    head = [int(rng.choice(P.full))]
    if k >= 4 and rng.random() < 0.5:
        head = [int(rng.choice(P.single)), int(rng.choice(np.flatnonzero(P.m >= k - 1)))]
    rest = [u for u in rng.permutation(np.concatenate([P.single[:4 * k], P.multi])) if u not in head][:k - len(head)]
    ids = np.asarray(head + sorted(int(u) for u in rest), dtype=np.int64)
    bits = np.concatenate([lv[:len(head)], np.full(k - len(head), lv[2], dtype=np.uint32)])
    return ids, bits


def _gen_slot0_tied(rng, P):
    """slot 0 a class that fills the list, slot 1 at the same distance: its representative follows slot 0's (the order
    of the list) but precedes most of slot 0's members, so the answer interleaves the two classes"""
    k = P.k
    if k < 2:
        return None
    early = P.full[P.full < P.size.size // 2]  # (a class of many rows has an early representative)
    u0 = int(rng.choice(early if early.size else P.full[:-1]))
    u1 = int(rng.integers(u0 + 1, min(u0 + 40, P.size.size)))
    lv = _levels(rng, 3)
    rest = [int(u) for u in rng.permutation(np.concatenate([P.single, P.multi])) if u not in (u0, u1)][:k - 2]
    ids, bits = _sorted([u0, u1] + rest, np.concatenate([[lv[0], lv[0]], rng.choice(lv[1:], k - 2)]))
    return ids, bits


GENERATORS = [_gen_fast, _gen_concat, _gen_tie(0, 32), _gen_fast, _gen_tie(32, 64), _gen_tie_behind, _gen_fast,
              _gen_tie(64, 128), _gen_slot0_tied, _gen_fast, _gen_tie(128, 1 << 30), _gen_concat]


def lists(members, k, seed):
    """One list per unique row: (ids int32 [nu, k], bits uint32 [nu, k]); the generators in turn, over a shuffled order
    of the unique rows (a generator that cannot make its stratum at this k passes its turn on)."""
    rng = np.random.default_rng(seed)
    P, nu = _Pools(members, k), len(members)
    ids, bits = np.empty((nu, k), dtype=np.int32), np.empty((nu, k), dtype=np.uint32)
    turn = 0
    for u in rng.permutation(nu):
        got = None
        while got is None:
            got = GENERATORS[turn % len(GENERATORS)](rng, P)
            turn += 1
        ids[u], bits[u] = got
    key = (bits.astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
    assert np.all(key[:, 1:] > key[:, :-1]) and ids.min() >= 0 and ids.max() < nu
    return ids, bits


def queries_per_wave(k):
    return (64 // k) * 4


def condition(k, paths_u, paths_q):
    """The floor, from path_of alone: every reachable stratum holds FLOOR lists (so at least FLOOR queries), and with
    two or more queries per wave pass FLOOR ballots (the 64 // k queries a wave handles at once) and FLOOR waves mix
    fast and other queries."""
    cu, cq = M.counts(paths_u), M.counts(paths_q)
    for s in M.STRATA:
        if s in M.reachable(k):
            assert cu[s] >= FLOOR and cq[s] >= FLOOR, (k, s, cu, cq)
        else:
            assert cu[s] == 0, (k, s, cu)
    mixed = {}
    for name, group in (("ballots", 64 // k), ("waves", queries_per_wave(k))):
        fast = np.array([np.sum(paths_q[a:a + group] == "fast") for a in range(0, len(paths_q), group)])
        full = np.array([len(paths_q[a:a + group]) for a in range(0, len(paths_q), group)])
        mixed[name] = int(np.sum((fast > 0) & (fast < full)))
        if group >= 2:
            assert mixed[name] >= FLOOR, (k, name, mixed)
    return cu, cq, mixed
