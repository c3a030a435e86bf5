"""The live-chunk candidate pass (knn_prefilter_live_kernel<NL>, fedrann_amd/csrc/knn_prefilter_live.inc): at d = 128,
k = 20, forced, in prefilter mode, on rows whose chunk masks are CHOSEN -- indices and distance bits against the CPU
oracle and against exact mode, and the work items per NL the trace reports against the masks.

Every row has a positive value at the first component of each chunk of its class (so its mask is exactly the class's
and any two rows that share a chunk have a positive similarity) and a few more positive values inside those chunks.
Every non-zero query therefore has far more than k rows of positive similarity (checked on the oracle's answer: the
k-th distance is below 1), so no case leans on the exact fallback for lack of candidates; the all-zero rows, the 200
equal one-component rows and the 40 copies of one row are there to take the zero / range ways on purpose.

The second half (from live_check on) reads the pass's OWN output: the captured candidate lists against the float64
model of tests/_candidate_model.py, as tests/test_gpu_candidates.py does for the other two candidate-pass kernels --
the prefilter mode heals a wrong list through the exact fallback, so final bits alone cannot see it.  Those rows are
signed (tests/_live_rows.py); the table above live_check says which instance, K', d and target-set shape each test
covers, and tests/test_candidate_model.py shows on the CPU that these inputs make a dropped chunk, swapped halves and a
neighbour's chunk ids fail the checks.
"""
import numpy as np
import pytest

import _candidate_model as M
import _live_rows as LR
from _live_rows import CLASSES, D, expected_blocks, expected_items, four_classes, rows_of  # noqa: F401
from _paths_rows import _normalize
from _strata import stratified_rows
from fedrann_amd import _lib
from test_gpu_candidates import _check, _kp, _run, _variant
from test_gpu_parity import _adversarial_rows

pytestmark = pytest.mark.gpu

K = 20


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
    tr, launches = ctx.last_knn_trace(), ctx.last_prefilter_launches()
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
    # 36 .. 52 query blocks, far below one round: every group in ONE launch, all on the caller's stream
    assert tr["pass_launches"] == sum(1 for v in items.values() if v != 0) and tr["pass_queues"] == 1, tr
    assert launches == (tr["pass_launches"], tr["pass_queues"]), (launches, tr)
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


# ---- the captured lists against the float64 model (tests/_candidate_model.py) ------------------------------------------
# Coverage (instance = knn_prefilter_live_kernel<NL>; "dense" = the gathered dense group; K' of k = 20 is 32):
#   test_lists_every_instance_dense_signed_rows   NL 2 (d 16, padded id; d 32), 3 (d 40, 48), 4, 5, 6 (d 64, 80, 96), dense
#                                                 (d 100); K' 32; 3 000 targets = 94 tiles, signed dense / sparse rows
#   test_lists_signed_mask_classes                NL 2 .. 6 and dense in one call, d 128, K' 32, 6 290 targets, lists that
#                                                 fill at d~ = 1, all-zero rows
#   test_lists_list_shapes                        K' 14, 32, 30, 32 (dead entries, odd halves); K' 38: FORCE refused
#   test_lists_small_target_sets                  NL 4 (d 64) and NL 2 (d 128): 1 .. 5 tiles and 9, nvalid < 32
#   test_lists_several_segments_and_query_blocks  the same two at 20 013 targets, several segments; rank-form query blocks
#                                                 of 1, 1, 33 and 257 rows with their own order table
#   test_lists_bit_identical_to_the_dense_pass    FORCE against OFF, d 64, 96 and the mask classes
#   test_auto_groups_at_the_size_of_rounds        AUTO, 1.15 x 512 x CUs rows: groups, padded joins, two queues
#   test_duplicate_layer_on_forced_live_pass      the duplicate-row layer (auto, force) over the forced pass
M_CERT = 2 * M.PREFILTER_EPS + 4e-7  # the certificate's margin M (knn_prefilter.inc)


def _with_live(ctx, mode, fn, *args, **kwargs):
    ctx.set_live_chunks(mode)
    try:
        return fn(ctx, *args, **kwargs)
    finally:
        ctx.set_live_chunks("auto")


def _items(tr):
    return {key: v for key, v in tr.items() if key.startswith("pass_live_")}


def _oracle_rows(oracle, E, rows, k, t_base=0):
    Eh, _, z = oracle.normalize(E)
    return oracle.knn_normalized(Eh[rows], z[rows], Eh, z, k, t_base=t_base)


def _device_rows(ctx, E):
    import torch
    return _normalize(ctx, torch.from_numpy(np.ascontiguousarray(E)).to("cuda"))


def live_check(ctx, oracle, E, q0, nq, k, t_base, tag, complete, want=None, mode="force"):
    """Rows [q0, q0 + nq) of E against all of E on the live-chunk pass: the captured lists against the model (_check:
    shape, accuracy, premise, completeness of `complete`), the trace's items against the device rows' masks, and the
    final indices and distance bits against the oracle (`want`: its answer for these queries, else computed here).
    Returns (report, trace, path codes)."""
    n, d = E.shape
    Ehat, zero = _device_rows(ctx, E)
    rep, tr = _with_live(ctx, mode, _check, Ehat, zero, q0, nq, d, k, t_base, tag, complete=complete)
    assert tr["pass_live"] == 1 and tr["pass_list_keys"] == 16, (tag, tr)
    X = Ehat[q0:q0 + nq].cpu().numpy()
    if mode == "force":
        assert _items(tr) == expected_items(X, tr["pass_segments"]), (tag, _items(tr), expected_blocks(X))
    idx, dst, paths, tr2, _, _, _ = _with_live(ctx, mode, _run, Ehat, zero, q0, nq, d, k, t_base, capture=0)
    assert tr2 == tr, (tag, tr2, tr)
    if want is None:
        want = _oracle_rows(oracle, E, q0 + np.arange(nq), k, t_base)
    assert same_bits((idx, dst), want), "%s: the forced live-chunk pass differs from the oracle" % tag
    return rep, tr, paths


SET1 = [(kind, d) for d in (16, 32, 48, 64, 80, 96, 40, 100) for kind in ("fp16_midpoints", "fp16_subnormals", "dense")]


def _set1(kind, d, n=3000):
    return _adversarial_rows(kind, n, d, np.random.default_rng(d + 7 * len(kind)))


@pytest.mark.parametrize("kind,d", SET1, ids=["%s-%d" % a for a in SET1])
def test_lists_every_instance_dense_signed_rows(ctx, oracle, kind, d):
    """3 000 signed rows that fill all ceil(d / 16) chunks, all-pairs, k = 20: d = 16 NL puts the 12 blocks on instance
    NL (d = 16: one chunk, run as two with a padded id; d = 40: three, the last half full; d = 100: seven, the dense
    kernel through live_gather_dense_kernel).  That holds for the dense kind, whose every row fills every chunk; the
    sparse kinds' first blocks -- their rows of fewest chunks (fp16_midpoints: six non-zeros a row) -- hold fewer
    chunks and run on smaller instances: the items are those of the device rows' own masks (live_check)."""
    E = _set1(kind, d)
    _, tr, _ = live_check(ctx, oracle, E, 0, 3000, K, 0, "set1/%s-%d" % (kind, d), np.arange(3000))
    nl, nseg = -(-d // 16), tr["pass_segments"]
    key = "pass_live_dense_items" if nl >= 7 else "pass_live_items_%d" % max(nl, 2)
    assert tr[key] > 0 and (kind != "dense" or tr[key] == 12 * nseg), (key, tr)


@pytest.fixture(scope="module")
def signed(oracle):
    """(E, kind, oracle idx, oracle dist) of the signed mask classes, 6 290 rows; on the CPU: every row but the lonely
    and the zero ones has its k-th neighbour (k = 24 too) so far below distance 1 that the certificate's first
    condition d~(K) + M < 1 holds whatever the pass rounds: d(K) + eps + M < 1."""
    E, kind = LR.signed_classes(np.random.default_rng(2209))
    E.setflags(write=False)
    idx, dist = oracle.knn(E, 24)
    assert np.all(dist[kind >= 2, 23] < 1.0 - (M_CERT + M.prefilter_eps(20))), dist[kind >= 2, 23].max()
    assert np.all(dist[kind == 1, K - 1] == 1.0)  # (a lonely row: ten equal rows, everything else at 1)
    idx, dist = oracle.knn(E, K)
    return E, kind, idx, dist


def test_lists_signed_mask_classes(ctx, oracle, signed):
    """Signed values, classes of 2 .. 6 chunks (every instance and the dense group in one call), 300 lonely rows whose
    lists fill at d~ = 1 -- fewer than K' targets of positive similarity, the certificate fails by design -- and 40
    all-zero rows.  At most those 340 rows may be left to the exact kernel: every other row is certified or a range
    row (its k-th distance is far enough below 1, see the fixture), so a fallback here is unexplained."""
    E, kind, idx, dist = signed
    n = E.shape[0]
    rep, tr, paths = live_check(ctx, oracle, E, 0, n, K, 0, "set2", np.arange(n), want=(idx, dist))
    for nl in range(2, 7):
        assert tr["pass_live_items_%d" % nl] > 0, tr
    code = paths & 0x7F
    assert np.all(code[kind == 1] == _lib.PATH_EXACT), np.unique(code[kind == 1])
    assert np.all(code[kind == 0] == _lib.PATH_ZERO)
    other = code[kind >= 2]
    assert np.all((other == _lib.PATH_CERTIFIED) | (other == _lib.PATH_RANGE)), np.unique(other, return_counts=True)
    assert tr["exact_queries"] <= 300 + 40 and tr["zero_queries"] == 40, tr


@pytest.mark.parametrize("k", (1, 20, 21, 24))
def test_lists_list_shapes(ctx, oracle, signed, k):
    """K' = 14, 32, 30, 32 on the first 3 000 rows of the mask classes: dead entries (2 x 9 and 2 x 1 of the halves' 16)
    and the full list."""
    E = signed[0][:3000]
    _, tr, _ = live_check(ctx, oracle, E, 0, 3000, k, 0, "shapes/k%d" % k, np.arange(3000))
    assert tr["kp"] == _kp(k) == {1: 14, 20: 32, 21: 30, 24: 32}[k], tr


def test_force_is_refused_beyond_32_keys(ctx, oracle, signed):
    """k = 25: K' = 38 takes 32-key lists, which the live-chunk pass does not have -- FORCE must not apply."""
    E = signed[0][:3000]
    Ehat, zero = _device_rows(ctx, E)
    _, tr = _with_live(ctx, "force", _check, Ehat, zero, 0, 3000, D, 25, 0, "shapes/k25", complete=np.arange(3000))
    assert tr["kp"] == 38 and tr["pass_live"] == 0 and tr["pass_list_keys"] == 32, tr
    assert all(v == 0 for v in _items(tr).values()), tr
    got = _with_live(ctx, "force", _run, Ehat, zero, 0, 3000, D, 25, 0, capture=0)
    assert same_bits(got[:2], _oracle_rows(oracle, E, np.arange(3000), 25))


def _edge_rows(variant, n, seed):
    """"d64": dense signed rows, every block on instance 4; "two_chunks": d = 128, signed, chunks 0 and 7 (instance 2)"""
    rng = np.random.default_rng(seed)
    if variant == "d64":
        return _adversarial_rows("dense", n, 64, rng)
    return LR.signed_rows_of((0, 7), n, rng)


@pytest.mark.parametrize("variant", ("d64", "two_chunks"))
def test_lists_small_target_sets(ctx, oracle, variant):
    """nt = K', 33, 65, 97, 129, 257 all-pairs: 1 .. 5 tiles (a last stage of one pair; an odd last pair whose second
    tile is padding; the late waves' MFMA-less last iteration scoring a pair of its own; nvalid < 32 in the last tile)
    and one row more than a query block.  Every check on every query."""
    for nt in (32, 33, 65, 97, 129, 257):
        E = _edge_rows(variant, nt, seed=nt)
        _, tr, _ = live_check(ctx, oracle, E, 0, nt, K, 0, "%s/nt%d" % (variant, nt), np.arange(nt))
        assert tr["kp"] == 32 and tr["pass_live_items_%d" % (4 if variant == "d64" else 2)] > 0, tr


@pytest.fixture(scope="module")
def edge_sets():
    return {v: _edge_rows(v, 20013, seed=5) for v in ("d64", "two_chunks")}


@pytest.mark.parametrize("variant", ("d64", "two_chunks"))
def test_lists_several_segments_and_query_blocks(ctx, oracle, edge_sets, variant):
    """20 013 targets (not a multiple of 32; several target segments under FORCE): all-pairs with every seventh list
    tested for completeness and compared with the oracle, then the rank form -- row numbers from 2^20, query blocks of
    1, 1, 33 and 257 rows (short and partial blocks with their own order table), every listed row inside
    [t_base, t_base + nt) (check_lists' shape check)."""
    E = edge_sets[variant]
    n = E.shape[0]
    Ehat, zero = _device_rows(ctx, E)
    d = E.shape[1]
    nl = "pass_live_items_%d" % (4 if variant == "d64" else 2)
    some = np.arange(0, n, 7)
    rep, tr = _with_live(ctx, "force", _check, Ehat, zero, 0, n, d, K, 0, "%s/n%d" % (variant, n), complete=some)
    assert tr["pass_live"] == 1 and tr["pass_segments"] > 1, tr
    assert _items(tr) == expected_items(Ehat.cpu().numpy(), tr["pass_segments"]) and tr[nl] > 0, tr
    got = _with_live(ctx, "force", _run, Ehat, zero, 0, n, d, K, 0, capture=0)
    wi, wd = _oracle_rows(oracle, E, some, K)
    assert same_bits((got[0][some], got[1][some]), (wi, wd)), variant
    for q0, nq in ((0, 1), (n - 1, 1), (5000, 33), (n - 257, 257)):
        tag = "%s/block%d+%d" % (variant, q0, nq)
        rep, tr = _with_live(ctx, "force", _check, Ehat, zero, q0, nq, d, K, 1 << 20, tag, complete=np.arange(nq))
        assert tr["pass_live"] == 1 and tr["queries"] == nq and tr["targets"] == n, tr
        assert _items(tr) == expected_items(Ehat[q0:q0 + nq].cpu().numpy(), tr["pass_segments"]), (tag, tr)
        got = _with_live(ctx, "force", _run, Ehat, zero, q0, nq, d, K, 1 << 20, capture=0)
        assert same_bits(got[:2], _oracle_rows(oracle, E, q0 + np.arange(nq), K, t_base=1 << 20)), tag


@pytest.mark.parametrize("name", ("dense-64", "dense-96", "mask-classes"))
def test_lists_bit_identical_to_the_dense_pass(ctx, signed, name):
    """knn_prefilter_live.inc: "the similarities are the dense pass's bit for bit" -- on the lists themselves: under
    FORCE and under OFF (the shape the planner picks at this size, printed) every query's sorted d~ bit patterns are
    equal, and so are the listed rows wherever d~ lies strictly below the list's last value (ties at the boundary may
    resolve differently: the two scans meet the targets in different order)."""
    E = signed[0] if name == "mask-classes" else _set1("dense", int(name[6:]))
    n, d = E.shape
    Ehat, zero = _device_rows(ctx, E)
    on = _with_live(ctx, "force", _run, Ehat, zero, 0, n, d, K, 0)
    off = _with_live(ctx, "off", _run, Ehat, zero, 0, n, d, K, 0)
    assert on[3]["pass_live"] == 1 and off[3]["pass_live"] == 0 and on[5] == off[5], (on[3], off[3])
    print("%s: OFF ran %s" % (name, _variant(off[3])))
    nz = np.flatnonzero(zero.cpu().numpy() == 0)
    ka, kb = np.sort(on[4][nz], axis=1), np.sort(off[4][nz], axis=1)
    da, db = (ka >> np.uint64(32)), (kb >> np.uint64(32))
    bad = np.flatnonzero((da != db).any(1))
    assert bad.size == 0, "%d queries' d~ bits differ from the dense pass (%s), first query %d: %s / %s" % (
        bad.size, _variant(off[3]), nz[bad[0]], da[bad[0]], db[bad[0]])
    inner = da < da[:, -1:]
    bad = np.flatnonzero(((ka != kb) & inner).any(1))
    assert bad.size == 0, "%d queries list other rows below the boundary, first query %d" % (bad.size, nz[bad[0]])


def _rounds_rows(n, rng):
    """The signed classes of 2, 4, 5 and 6 chunks scaled up to n rows with 40 all-zero rows, and ONE small three-chunk
    class: 300 rows on chunks {1, 4, 6}.  It contains the two-chunk class's {1, 6}, so whether a 256-row block lies
    inside it or straddles the two-chunk class's end, some block has exactly three live chunks -- one or two blocks,
    far fewer work items than a round."""
    rest = n - 340
    share = np.array([LR.SIGNED_SIZES[i] for i in (0, 2, 3, 4)], dtype=np.float64)
    sizes = np.floor(share / share.sum() * rest).astype(np.int64)
    sizes[0] += rest - sizes.sum()
    parts = [LR.signed_rows_of(LR.SIGNED_CHUNKS[i], int(m), rng) for i, m in zip((0, 2, 3, 4), sizes)]
    parts += [LR.signed_rows_of((1, 4, 6), 300, rng), np.zeros((40, D), dtype=np.float32)]
    E = np.concatenate(parts)
    return np.ascontiguousarray(E[rng.permutation(n)])


def test_auto_groups_at_the_size_of_rounds(ctx, oracle):
    """AUTO at 1.15 x 512 x CUs rows (CASES' d128_w8u4_rounds), on rows WITH live chunks: several groups launched in
    rounds on two queues, and a group smaller than one round -- the three-chunk blocks -- joining instance 4 with
    padded chunk ids.  The lists of a stratified sample (>= 256 complete, first and last row) against the model; the
    final bits of the sampled rows against the oracle."""
    n = int(1.15 * 512 * ctx.device_info()["cus"])
    E = _rounds_rows(n, np.random.default_rng(2210))
    Ehat, zero = _device_rows(ctx, E)
    rep, tr = _with_live(ctx, "auto", _check, Ehat, zero, 0, n, D, K, 0, "auto-rounds")
    assert tr["pass_live"] == 1, "AUTO did not take the live-chunk pass at n = %d: %s" % (n, tr)
    assert tr["pass_queues"] == 2 and tr["pass_launches"] > 2, tr
    nqb = -(-n // 256)
    assert sum(_items(tr).values()) == nqb * tr["pass_segments"], (tr, nqb)
    blocks = expected_blocks(Ehat.cpu().numpy())
    assert (blocks == 3).sum() > 0, "the input has no block of three live chunks: %s" % np.bincount(blocks)
    assert tr["pass_live_items_3"] == 0, "the three-chunk blocks (%d of them, %d segments) ran as a group of their " \
        "own: the premise that they are fewer than a round does not hold on this device: %s" % (
            (blocks == 3).sum(), tr["pass_segments"], tr)
    assert tr["pass_live_items_4"] >= ((blocks == 3).sum() + (blocks == 4).sum()) * tr["pass_segments"], tr
    idx, dst, paths, tr2, _, _, _ = _with_live(ctx, "auto", _run, Ehat, zero, 0, n, D, K, 0, capture=0)
    assert ctx.last_prefilter_launches() == (tr["pass_launches"], 2) and tr2 == tr
    rows, _, _ = stratified_rows(paths, per=64, seed=4)
    rows = np.unique(np.concatenate([rows, [0, n - 1]]))
    assert same_bits((idx[rows], dst[rows]), _oracle_rows(oracle, E, rows, K))


@pytest.mark.parametrize("dedup", ("auto", "force"))
def test_duplicate_layer_on_forced_live_pass(live, sets, dedup):
    """the duplicate-row layer on top of the forced pass (the all-zero rows, the 200 equal rows and the 40 copies form
    classes): the oracle's bits"""
    E, idx, dist = sets["with_extras"]
    live.set_dedup_mode(dedup)
    got = live.knn(E, K)
    tr = live.last_knn_trace()
    assert tr["kind"] == "prefilter" and tr["pass_live"] == 1, tr
    assert same_bits(got, (idx, dist))
