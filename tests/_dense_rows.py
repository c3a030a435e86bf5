"""Dense embedding rows on which the fp32 summation order shows in the distance bits.

The sparse rows of the older k-NN tests (six non-zeros a row) give dot products of at most a few non-zero terms, whose
fp32 result hardly depends on the order of the chain or on where it is split.  The rows here are dense and correlated,
so that distances sit well below 1 (near 1 the rounding of 1 - c hides the low bits of c) and every dot product is a
long chain of terms that cancel or nearly cancel.  tests/test_dense_rows.py checks, with the oracle's own pair
distance, that a changed summation order changes the distance bits of a large share of their pairs.

    cancel    one shared direction with mixed signs and magnitudes log-uniform over 2^-12 .. 2^12, each row perturbed
              by a few per cent: distances near 0, heavy cancellation in every dot product
    clusters  dense clusters of near-duplicates whose members lie a few ulps of c apart (the k-th and (k+1)-th
              neighbours differ by a few ulps), plus exact duplicates of dense rows placed far apart in row order
              (they land in different target segments: ties broken by index across the merge)
    halves    rows whose non-zeros lie only below component `split` (512 above d = 512, the split-K kernel's
              hand-off), only at or above it, or across it; at d = 513 also rows whose only non-zero is component 512
    zero rows mixed into each of them

mixed() stacks all three in one set and reports the rows worth sampling."""
import numpy as np

GENERATORS = ("cancel", "clusters", "halves")


def _logmag(rng, shape, span=12.0):
    """Random signs times magnitudes log-uniform over 2^-span .. 2^span."""
    return rng.choice([-1.0, 1.0], size=shape) * np.exp2(rng.uniform(-span, span, size=shape))


def _zeros(E, rng, frac=0.02):
    n = E.shape[0]
    if n:
        E[rng.choice(n, size=max(1, int(frac * n)), replace=False)] = 0.0
    return E


def cancel(n, d, seed, noise=0.05, zero_frac=0.02):
    rng = np.random.default_rng(seed)
    base = _logmag(rng, d)
    E = base[None, :] * (1.0 + noise * rng.standard_normal((n, d)))
    E *= np.exp2(rng.uniform(-4.0, 4.0, size=(n, 1)))  # (row scale: normalisation takes it out again)
    return _zeros(E.astype(np.float32), rng, zero_frac)


def clusters(n, d, seed, size=160, spread=2.0 ** -11, zero_frac=0.02, dups=16):
    """Clusters of `size` members (size > k + 1 for every k <= 128: the k-th neighbour boundary falls inside one)."""
    rng = np.random.default_rng(seed)
    nc = max(1, -(-n // size))
    centers = rng.standard_normal((nc, d)) * (1.0 + 0.5 * _logmag(rng, (1, d), 2.0))
    which = np.arange(n) % nc  # (members interleaved over the whole row range)
    E = centers[which] * (1.0 + spread * rng.standard_normal((n, d)))
    E = _zeros(E.astype(np.float32), rng, zero_frac)
    # exact duplicates of dense rows, half the set apart
    for i in rng.choice(n // 2, size=min(dups, n // 2), replace=False):
        E[i + n // 2] = E[i]
    return E


def halves(n, d, seed, zero_frac=0.02):
    rng = np.random.default_rng(seed)
    s = 512 if d > 512 else max(1, d // 2)
    lo, hi = max(0, s - 64), min(d, s + 64)
    spans = [(0, s), (s, d), (lo, hi)]
    E = np.zeros((n, d), np.float32)
    part = rng.integers(0, 3, size=n)
    for p, (a, b) in enumerate(spans):
        rows = np.flatnonzero(part == p)
        if rows.size == 0 or b <= a:
            continue
        base = _logmag(rng, b - a, 6.0)
        E[rows, a:b] = base[None, :] * (1.0 + 0.1 * rng.standard_normal((rows.size, b - a)))
    if d == 513:  # the last component alone: the split-K hand-off and the padding to 1024
        single = rng.choice(n, size=max(2, n // 64), replace=False)
        E[single] = 0.0
        E[single, 512] = rng.uniform(0.5, 2.0, size=single.size) * rng.choice([-1.0, 1.0], size=single.size)
    return _zeros(E, rng, zero_frac)


def make(kind, n, d, seed):
    return {"cancel": cancel, "clusters": clusters, "halves": halves}[kind](n, d, seed)


def mixed(n, d, seed, k=128):
    """The three generators stacked into one set of n rows (cancel | clusters | halves, a third each), with exact
    duplicates of cancel rows placed in the last third.  Returns (E, rows worth sampling: cluster members around the
    boundaries and duplicate pairs)."""
    rng = np.random.default_rng(seed)
    a, b = n // 3, 2 * n // 3
    E = np.concatenate([cancel(a, d, seed + 1), clusters(b - a, d, seed + 2, size=max(k + 32, 160)),
                        halves(n - b, d, seed + 3)])
    src = rng.choice(a, size=8, replace=False)
    dst = b + rng.choice(n - b, size=8, replace=False)
    E[dst] = E[src]
    interesting = np.concatenate([src, dst, a + np.arange(0, min(24, b - a)), rng.choice(np.arange(a, b), 16)])
    return np.ascontiguousarray(E), np.unique(interesting)


def sample_rows(n, seed, extra=(), per=48):
    """Query rows worth checking: both ends, rows around multiples of 32, 64 and 128 (the tile, wave and workgroup
    edges), `extra` and `per` random rows."""
    rng = np.random.default_rng(seed)
    edges = [0, 1, 2, n - 3, n - 2, n - 1]
    for m in (32, 64, 128):
        for c in rng.choice(np.arange(m, n, m), size=min(4, max(0, (n - 1) // m)), replace=False):
            edges += [c - 1, c, c + 1]
    rows = np.concatenate([np.asarray(edges), np.asarray(extra, dtype=np.int64), rng.choice(n, size=min(per, n),
                                                                                           replace=False)])
    rows = rows[(rows >= 0) & (rows < n)]
    return np.unique(rows).astype(np.int64)


def order_sensitivity(oracle, E, pairs, perm):
    """Share of the pairs (i, j) whose canonical distance bits change when both rows' components are summed in the
    order `perm` instead of ascending."""
    Eh, _, zero = oracle.normalize(E)
    changed = 0
    for i, j in pairs:
        a = oracle.pair_dist_normalized(Eh[i], zero[i], Eh[j], zero[j])
        b = oracle.pair_dist_normalized(Eh[i][perm], zero[i], Eh[j][perm], zero[j])
        changed += np.float32(a).view(np.uint32) != np.float32(b).view(np.uint32)
    return changed / max(1, len(pairs))
