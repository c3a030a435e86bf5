"""The live-chunk candidate pass (knn_prefilter_live_kernel<NL>, fedrann_amd/csrc/knn_prefilter_live.inc): at d = 128,
k = 20, forced, in prefilter mode, on rows whose chunk masks are CHOSEN -- indices and distance bits against the CPU
oracle and against exact mode, and the work items per NL the trace reports against the masks.

Every row has a positive value at the first component of each chunk of its class (so its mask is exactly the class's
and any two rows that share a chunk have a positive similarity) and a few more positive values inside those chunks.
Every non-zero query therefore has far more than k rows of positive similarity (checked on the oracle's answer: the
k-th distance is below 1), so no case leans on the exact fallback for lack of candidates; the all-zero rows, the 200
equal one-component rows and the 40 copies of one row are there to take the zero / range ways on purpose.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, K = 128, 20
CLASSES = (((1, 6), 3000), ((0, 2, 5), 3100), ((0, 1, 3, 4, 7), 3050), ((1, 2, 3, 5, 6, 7), 3138))  # 12 288 rows


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


def expected_blocks(E):
    """NL of every 256-row query block: the rows in (non-empty chunks, mask) order, stable, as the library scans them."""
    m = ((E != 0).reshape(E.shape[0], 8, 16).any(2) * (1 << np.arange(8))).sum(1).astype(np.int64)
    cnt = np.unpackbits(m.astype(np.uint8)[:, None], axis=1).sum(1).astype(np.int64)
    ms = m[np.argsort((cnt << 32) | m, kind="stable")]
    ms = np.concatenate([ms, np.zeros((-ms.size) % 256, dtype=np.int64)]).reshape(-1, 256)
    u = np.bitwise_or.reduce(ms, axis=1)
    return np.unpackbits(u.astype(np.uint8)[:, None], axis=1).sum(1)


def expected_items(E, nseg):
    """the trace's item counts: blocks below two live chunks run as two, seven and eight on the dense kernel"""
    nl = np.maximum(expected_blocks(E), 2)
    want = {"pass_live_items_%d" % n: int((nl == n).sum()) * nseg for n in range(2, 7)}
    want["pass_live_dense_items"] = int((nl >= 7).sum()) * nseg
    return want


@pytest.fixture(scope="module")
def sets(oracle):
    """name -> (E, oracle idx, oracle dist): computed once, never modified"""
    rng = np.random.default_rng(2207)
    out = {}
    out["one_chunk"] = rows_of((3,), 9000, rng)
    base = four_classes(rng)
    out["four_classes"] = base[rng.permutation(base.shape[0])]
    one = np.zeros((200, D), dtype=np.float32)
    one[:, 16] = rng.uniform(0.5, 2.0, size=200)  # (one normalised row, 200 times)
    extra = np.concatenate([base, np.zeros((300, D), dtype=np.float32), one, np.repeat(base[4000:4001], 40, axis=0)])
    out["with_extras"] = extra[rng.permutation(extra.shape[0])]
    out["partial_tile"] = rows_of((0, 7), 8192 + 13, rng)
    res = {}
    for name, E in out.items():
        E = np.ascontiguousarray(E)
        E.setflags(write=False)
        idx, dist = oracle.knn(E, K)
        nz = np.abs(E).sum(1) > 0
        assert np.all(dist[nz, K - 1] < 1.0), name  # >= k rows of positive similarity for every non-zero query
        res[name] = (E, idx, dist)
    return res


@pytest.fixture()
def live(ctx):
    """prefilter mode, the duplicate-row layer off (every row reaches the pass), live chunks forced; restored afterwards"""
    ctx.set_knn_mode("prefilter")
    ctx.set_dedup_mode("off")
    ctx.set_live_chunks("force")
    yield ctx
    ctx.set_live_chunks("auto")
    ctx.set_dedup_mode("auto")
    ctx.set_knn_mode("auto")


def same_bits(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def run_forced(ctx, E, want):
    got = ctx.knn(E, K)
    tr = ctx.last_knn_trace()
    assert tr["kind"] == "prefilter" and tr["pass_live"] == 1 and tr["pass_waves"] == 8 and tr["pass_units"] == 8, tr
    assert same_bits(got, want), "forced live-chunk pass differs from the oracle"
    ctx.set_knn_mode("exact")
    try:
        exact = ctx.knn(E, K)
    finally:
        ctx.set_knn_mode("prefilter")
    assert same_bits(got, exact), "forced live-chunk pass differs from exact mode"
    items = {k: v for k, v in tr.items() if k.startswith("pass_live_") and k != "pass_live"}
    assert items == expected_items(E, tr["pass_segments"]), (items, expected_blocks(E))
    return tr


def test_one_live_chunk_runs_as_two(live, sets):
    """9 000 rows (36 blocks, the last one short), every non-zero in chunk 3: NL = 1 runs as 2 with a padded id"""
    E, idx, dist = sets["one_chunk"]
    tr = run_forced(live, E, (idx, dist))
    assert tr["pass_live_items_2"] == 36 * tr["pass_segments"] and tr["pass_live_dense_items"] == 0, tr


def test_four_mask_classes_and_straddling_blocks(live, sets):
    """12 288 rows, NL = 2, 3, 5, 6; the class sizes are no multiples of 256, so three blocks straddle two classes and
    take the union: {1,6} + {0,2,5} = 5 chunks, {0,2,5} + {0,1,3,4,7} = 7 and {0,1,3,4,7} + {1,2,3,5,6,7} = 8 -- the
    last two come out of the dense kernel, as two separate runs of blocks"""
    E, idx, dist = sets["four_classes"]
    tr = run_forced(live, E, (idx, dist))
    assert tr["pass_live_dense_items"] == 2 * tr["pass_segments"], tr
    for nl in (2, 3, 5, 6):
        assert tr["pass_live_items_%d" % nl] > 0, tr
    assert tr["pass_live_items_4"] == 0, tr


def test_zero_rows_duplicates_and_a_plateau(live, sets):
    """the same + 300 all-zero rows (a block without any live chunk), 200 equal one-component rows, 40 copies of a row"""
    E, idx, dist = sets["with_extras"]
    tr = run_forced(live, E, (idx, dist))
    assert tr["zero_queries"] == 300 and tr["range_queries"] + tr["uncertified"] > 0, tr


def test_partial_last_tile_first_and_last_chunk(live, sets):
    """8 205 rows (the last tile holds 13), live chunks {0, 7}: first and last piece of a tile, rows past the end"""
    E, idx, dist = sets["partial_tile"]
    tr = run_forced(live, E, (idx, dist))
    assert tr["pass_live_items_2"] == 33 * tr["pass_segments"], tr


def test_query_block_of_the_targets_on_device_pointers(live, sets):
    """queries != targets: rows [5000, 7048) of the four-class set against all of it, as a rank calls it -- the
    queries' own order and the targets' order both apply"""
    import torch
    from fedrann_amd.distributed import HipEngine
    E, idx, dist = sets["four_classes"]
    n, lo, nq = E.shape[0], 5000, 2048
    dev = torch.device("cuda", 0)
    eng = HipEngine(live, dev)
    dE = torch.from_numpy(E.copy()).to(dev)
    Ehat = torch.empty_like(dE)
    zero = torch.empty(n, dtype=torch.uint8, device=dev)
    eng.normalize(dE, Ehat, zero)
    g_idx, g_dst = eng.knn(Ehat[lo:lo + nq], zero[lo:lo + nq], nq, Ehat, zero, n, D, K)
    torch.cuda.synchronize(dev)
    tr = live.last_knn_trace()
    assert tr["pass_live"] == 1 and tr["queries"] == nq and tr["targets"] == n, tr
    assert same_bits((g_idx.cpu().numpy(), g_dst.cpu().numpy()), (idx[lo:lo + nq], dist[lo:lo + nq]))
    items = {k: v for k, v in tr.items() if k.startswith("pass_live_") and k != "pass_live"}
    assert items == expected_items(E[lo:lo + nq], tr["pass_segments"]), items


def test_auto_and_off_take_the_shipped_kernel_with_the_same_bits(live, sets):
    """below the size of synchronised rounds AUTO does not group; OFF never does; OFF and FORCE give the same bits"""
    E, idx, dist = sets["four_classes"]
    forced = live.knn(E, K)
    assert live.last_knn_trace()["pass_live"] == 1
    for mode in ("auto", "off"):
        live.set_live_chunks(mode)
        got = live.knn(E, K)
        tr = live.last_knn_trace()
        assert tr["kind"] == "prefilter" and tr["pass_live"] == 0 and tr["pass_live_dense_items"] == 0, (mode, tr)
        assert same_bits(got, forced) and same_bits(got, (idx, dist)), mode
