"""Rows with CHOSEN chunk masks for the live-chunk candidate pass (tests/test_gpu_live_chunks.py, and the CPU half in
tests/test_candidate_model.py), and what the library's planner makes of them: the scan order (knn_order.inc), the
256-row query blocks' masks (live_block_masks_kernel) and the per-instance work items (live_plan without a minimum
group size, as FORCE runs it).  Numpy only."""
import numpy as np

D = 128
CLASSES = (((1, 6), 3000), ((0, 2, 5), 3100), ((0, 1, 3, 4, 7), 3050), ((1, 2, 3, 5, 6, 7), 3138))  # 12 288 rows
# five signed classes of 2 .. 6 chunks, none of them on chunk 4: that one belongs to the lonely rows alone
SIGNED_CHUNKS = ((1, 6), (0, 2, 5), (2, 3, 5, 7), (0, 1, 3, 6, 7), (0, 1, 2, 3, 5, 7))
LONELY_CHUNK = 4
SIGNED_SIZES = (1130, 1190, 1250, 1170, 1210)  # no multiples of 256; 5 950 rows, 6 290 with the lonely and zero rows


def rows_of(chunks, n, rng, extra=3):
    """n rows, non-zero exactly inside `chunks` (every chunk's first component, + `extra` random components)."""
    E = np.zeros((n, D), dtype=np.float32)
    comps = np.concatenate([np.arange(16 * c, 16 * c + 16) for c in chunks])
    for c in chunks:
        E[:, 16 * c] = rng.uniform(0.2, 1.0, size=n)
    for _ in range(extra):
        E[np.arange(n), rng.choice(comps, size=n)] = rng.uniform(0.2, 1.0, size=n)
    return E


def four_classes(rng):
    return np.concatenate([rows_of(ch, n, rng) for ch, n in CLASSES])


def signed_rows_of(chunks, n, rng, extra=3):
    """rows_of with a random sign on every value: similarities of both signs, partial sums that change sign from one
    chunk to the next, and the clamp at 0 for about half the pairs that share a chunk."""
    E = rows_of(chunks, n, rng, extra)
    return E * rng.choice(np.float32([-1.0, 1.0]), size=E.shape)


def lonely_rows(n):
    """n rows +- e_j, j the 16 components of LONELY_CHUNK in turn, the sign changing every 16 rows: 32 groups of n / 32
    equal rows.  A lonely query has its own group at similarity 1 (fewer than K' rows as long as n < 32 K'), the
    opposite group at -1 and every other row at exactly 0: its list fills at d~ = 1 and the certificate fails."""
    E = np.zeros((n, D), dtype=np.float32)
    i = np.arange(n)
    E[i, 16 * LONELY_CHUNK + i % 16] = np.where((i // 16) % 2 == 0, 1.5, -0.75)
    return E


def signed_classes(rng, sizes=SIGNED_SIZES, lonely=300, zeros=40, shuffle=True):
    """The signed classes at `sizes` rows, `lonely` lonely rows and `zeros` all-zero rows.  Returns (E, kind): kind[i]
    = the number of chunks of row i's class (2 .. 6), 1 for a lonely row, 0 for an all-zero one."""
    parts = [signed_rows_of(ch, n, rng) for ch, n in zip(SIGNED_CHUNKS, sizes)]
    kind = [np.full(n, len(ch)) for ch, n in zip(SIGNED_CHUNKS, sizes)]
    parts += [lonely_rows(lonely), np.zeros((zeros, D), dtype=np.float32)]
    kind += [np.full(lonely, 1), np.zeros(zeros, dtype=np.int64)]
    E, kind = np.concatenate(parts), np.concatenate(kind)
    if shuffle:
        p = rng.permutation(E.shape[0])
        E, kind = E[p], kind[p]
    return np.ascontiguousarray(E), kind


def chunk_masks(X):
    """bit c of row i's mask <=> chunk c (components 16 c .. 16 c + 15) of X[i] holds a non-zero (-0.0 is none).  X: the
    rows as given (d <= 128 columns) or the device's normalised rows (128 columns; its component order permutes inside
    groups of 8 only, so the chunks are the same) -- the latter is what the library looks at (row_chunk_keys_kernel)."""
    X = np.asarray(X)
    n, d = X.shape
    assert d <= D, d
    nz = np.zeros((n, D), dtype=bool)
    nz[:, :d] = X != 0
    return (nz.reshape(n, 8, 16).any(2) * (1 << np.arange(8))).sum(1).astype(np.int64)


def _popcount8(m):
    return np.unpackbits(np.asarray(m).astype(np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def scan_order(X):
    """the rows in (non-empty chunks, mask) order, stable, as the library scans them (knn_order.inc)"""
    m = chunk_masks(X)
    return np.argsort((_popcount8(m) << 32) | m, kind="stable")


def block_masks(X):
    """the union mask of every 256-row block of the scan order (the last block may be short)"""
    ms = chunk_masks(X)[scan_order(X)]
    ms = np.concatenate([ms, np.zeros((-ms.size) % 256, dtype=np.int64)]).reshape(-1, 256)
    return np.bitwise_or.reduce(ms, axis=1)


def expected_blocks(X):
    """NL of every 256-row query block: the number of chunks that are non-empty in some row of the block."""
    return _popcount8(block_masks(X))


def expected_items(X, nseg):
    """the trace's item counts: blocks below two live chunks run as two, seven and eight on the dense kernel"""
    nl = np.maximum(expected_blocks(X), 2)
    want = {"pass_live_items_%d" % n: int((nl == n).sum()) * nseg for n in range(2, 7)}
    want["pass_live_dense_items"] = int((nl >= 7).sum()) * nseg
    return want


def block_ids(X):
    """live_plan without a minimum group size, per block of the scan order: the chunk ids its kernel multiplies,
    ascending -- the block's own, padded to two with the lowest empty chunks; all eight from seven live chunks on."""
    out = []
    for m in block_masks(X):
        m = int(m)
        pc = bin(m).count("1")
        if pc > 6:
            m = 0xFF
        for c in range(8):
            if bin(m).count("1") >= 2:
                break
            m |= 1 << c
        out.append([c for c in range(8) if (m >> c) & 1])
    return out
