"""Stage skipping of the live-chunk candidate pass (live_stage_masks_kernel, live_stage_lists_kernel and the list walk
of knn_prefilter_live_kernel<NL>, fedrann_amd/csrc/knn_prefilter_live.inc): a work item visits stage 0 of its segment
and the stages -- 128 rows of the scan order, counted from the segment's first row -- whose rows share a chunk with
the query block's mask.  d = 128, k = 20, prefilter mode, the duplicate-row layer off, live chunks forced; rows with
CHOSEN chunk sets (tests/_live_rows.py).

Every case checks (skip_check):
  * the final indices and distance bits against the CPU oracle;
  * against the same call with the switch off: every query's sorted d~ bit patterns are equal, and so are the listed
    rows wherever d~ lies strictly below the list's last value (ties at the boundary may resolve differently);
  * the trace's walked and skipped stage counts against the counts computed here from the device rows' masks, the
    scan order and the segments' first rows;
  * the device-built lists and lengths of every segment, for all 256 mask values, against the same model.
"""
import numpy as np
import pytest

import _live_rows as LR
from _guarded import knn_dev_guarded
from fedrann_amd import _lib
from test_gpu_candidates import CAPTURE
from test_gpu_live_chunks import _device_rows, _oracle_rows, same_bits
from test_gpu_parity import _adversarial_rows

pytestmark = pytest.mark.gpu

K = 20
D = LR.D
KEY_INF = np.uint64(0x7F800000FFFFFFFF)  # an empty slot of a captured candidate list


def _call(ctx, Ehat, zero, q0, nq, t_base, skip):
    """fdr_knn_dev of rows [q0, q0 + nq) against all rows with the switch at `skip`.  Returns (idx, dist, paths, trace,
    keys, tables); tables[g] = (first row, lens[256], lists[256, stages]) of target segment g (the context's
    own copy: read after the workspace is freed)."""
    import torch
    ctx.set_knn_mode("prefilter")
    ctx.set_dedup_mode("off")
    ctx.set_live_chunks("force")
    ctx.set_live_skip(skip)
    ctx.set_knn_capture(CAPTURE | _lib.CAPTURE_LIVE_LISTS)
    try:
        # (workspace and outputs hold 0xFF bytes between canaries, checked after the synchronise: tests/_guarded.py)
        idx, dst, ws = knn_dev_guarded(ctx, Ehat, zero, q0, nq, t_base, D, K)
        paths = ctx.last_query_paths(nq)
        tr = ctx.last_knn_trace()
        assert tr["kind"] == "prefilter" and tr["pass_live"] == 1, tr
        del ws
        torch.cuda.empty_cache()
        tables = [ctx.last_live_stage_lists(g) for g in range(tr["pass_segments"])]
        keys, _ = ctx.last_candidates(nq, tr["kp"])
    finally:
        ctx.set_knn_capture(0)
        ctx.set_live_skip("auto")
        ctx.set_live_chunks("auto")
        ctx.set_dedup_mode("auto")
        ctx.set_knn_mode("auto")
    return idx.cpu().numpy(), dst.cpu().numpy(), paths, tr, keys, tables


def model_tables(T, firsts, skip=True):
    """What the builder must make of the device's target rows T and the segments' first rows: per segment (stage
    masks, lens[256], lists: a list of 256 arrays) -- stage 0 and every stage whose rows share a chunk with the value."""
    ms = LR.chunk_masks(T)[LR.scan_order(T)]
    ends = list(firsts[1:]) + [ms.size]
    out = []
    for b, e in zip(firsts, ends):
        e = min(e, ms.size)
        nst = -(-(e - b) // 128) if e > b else 0
        sm = np.array([np.bitwise_or.reduce(ms[b + 128 * s:min(b + 128 * s + 128, e)]) for s in range(nst)], dtype=np.int64)
        lists = []
        for v in range(256):
            keep = (sm & v) != 0 if skip else np.ones(nst, dtype=bool)
            if nst:
                keep[0] = True
            lists.append(np.flatnonzero(keep))
        out.append((sm, np.array([li.size for li in lists]), lists))
    return out


def model_counts(Q, tables):
    """(walked, skipped) over the work items of the NL instances: the query blocks of at most six live chunks"""
    walked = skipped = 0
    for m in LR.block_masks(Q):
        if bin(int(m)).count("1") > 6:
            continue
        for sm, lens, _ in tables:
            walked += int(lens[int(m)])
            skipped += int(sm.size - lens[int(m)])
    return walked, skipped


def check_tables(tables, model, tag):
    for g, ((_, lens, lists), (sm, mlens, mlists)) in enumerate(zip(tables, model)):
        assert lists.shape == (256, sm.size), (tag, g, lists.shape, sm.size)
        assert np.array_equal(lens, mlens), (tag, g, np.flatnonzero(lens != mlens)[:8])
        for v in range(256):
            assert np.array_equal(lists[v, :lens[v]], mlists[v]), (tag, g, v, lists[v, :lens[v]], mlists[v])
            assert np.all(lists[v, lens[v]:] == 0xFFFF), (tag, g, v)


def same_lists(on, off, zero_rows, tag):
    """the captured keys (d~ bits << 32 | row) of two calls: equal sorted d~ patterns, equal rows below the boundary"""
    nz = np.flatnonzero(~zero_rows)
    ka, kb = np.sort(on[nz], axis=1), np.sort(off[nz], axis=1)
    da, db = ka >> np.uint64(32), kb >> np.uint64(32)
    bad = np.flatnonzero((da != db).any(1))
    assert bad.size == 0, "%s: %d queries' d~ bits differ with the switch off, first query %d: %s / %s" % (
        tag, bad.size, nz[bad[0]], da[bad[0]], db[bad[0]])
    inner = da < da[:, -1:]
    bad = np.flatnonzero(((ka != kb) & inner).any(1))
    assert bad.size == 0, "%s: %d queries list other rows below the boundary, first query %d" % (tag, bad.size, nz[bad[0]])


def skip_check(ctx, oracle, E, q0, nq, t_base, tag, dev=None):
    """One call with the switch on and one with it off, and every check of the module's docstring.  Returns (on, off,
    model tables, device query rows)."""
    Ehat, zero = dev if dev is not None else _device_rows(ctx, E)
    on = _call(ctx, Ehat, zero, q0, nq, t_base, "auto")
    off = _call(ctx, Ehat, zero, q0, nq, t_base, "off")
    want = _oracle_rows(oracle, E, q0 + np.arange(nq), K, t_base)
    assert same_bits(on[:2], want), "%s: the skipping pass differs from the oracle" % tag
    assert same_bits(off[:2], want), "%s: the pass with the switch off differs from the oracle" % tag
    same_lists(on[4], off[4], zero.cpu().numpy()[q0:q0 + nq] != 0, tag)
    T = Ehat.cpu().numpy()
    Q = T[q0:q0 + nq]
    firsts = [t[0] for t in on[5]]
    assert firsts == [t[0] for t in off[5]] and firsts[0] == 0 and all(f % 32 == 0 for f in firsts), (tag, firsts)
    model = model_tables(T, firsts)
    check_tables(on[5], model, tag)
    check_tables(off[5], model_tables(T, firsts, skip=False), tag + "/off")
    walked, skipped = model_counts(Q, model)
    tr, tro = on[3], off[3]
    print("%s: %d segments, stages walked %d, skipped %d (model %d, %d)" % (
        tag, tr["pass_segments"], tr["skip_stages_walked"], tr["skip_stages_skipped"], walked, skipped))
    assert tr["skip_live"] == 1 and (tr["skip_stages_walked"], tr["skip_stages_skipped"]) == (walked, skipped), (tag, tr)
    assert tro["skip_live"] == 0 and (tro["skip_stages_walked"], tro["skip_stages_skipped"]) == (walked + skipped, 0), (tag, tro)
    return on, off, model, Q


def _lonely_rows(n):
    """n rows +- e_j, j = components 72 .. 79 (the upper half of chunk 4) in turn, the sign changing every 8 rows: 16
    groups of about n / 16 equal rows (fewer than K' for n < 512).  _classes clears these components in every class row,
    so a lonely query has its own group at similarity 1, the opposite group at -1 and every other row at exactly 0."""
    E = np.zeros((n, D), dtype=np.float32)
    i = np.arange(n)
    E[i, 72 + i % 8] = np.where((i // 8) % 2 == 0, 1.5, -0.75)
    return E


def _classes(rng, spec, lonely=0, zeros=0, shuffle=True):
    parts = [LR.signed_rows_of(ch, n, rng) for ch, n in spec]
    if lonely:
        for part in parts:
            part[:, 72:80] = 0.0  # (component 64 keeps chunk 4 in the mask of the classes that hold it)
        parts.append(_lonely_rows(lonely))
    if zeros:
        parts.append(np.zeros((zeros, D), dtype=np.float32))
    E = np.concatenate(parts)
    if shuffle:
        E = E[rng.permutation(E.shape[0])]
    return np.ascontiguousarray(E)


DISJOINT = (((0, 1), 1510), ((2, 3), 1450), ((4, 5, 6), 1530), ((0, 7), 1490))  # no multiples of 128; 5 980 rows


def _mask(chunks):
    return sum(1 << c for c in chunks)


def test_disjoint_classes(ctx, oracle):
    """Four classes of which only {0,1} and {0,7} share a chunk, and 300 lonely rows on chunk 4 whose lists fill at
    d~ = 1 (fewer than K' rows of positive similarity: _lonely_rows).  The class sizes are no multiples of 128, so stages straddle
    two classes: such a stage is on the list of either class's blocks.  The device lists of all 256 mask values are
    checked against the model (skip_check): this is the builder's test as well."""
    E = _classes(np.random.default_rng(2601), DISJOINT, lonely=300)
    on, _, model, _ = skip_check(ctx, oracle, E, 0, E.shape[0], 0, "disjoint")
    tr = on[3]
    assert tr["skip_stages_skipped"] > 0, tr
    straddling = 0
    for (_, lens, lists), (sm, _, _) in zip(on[5], model):
        for s in np.flatnonzero((sm == _mask((0, 1)) | _mask((2, 3))) | (sm == _mask((2, 3)) | _mask((0, 7)))):
            straddling += 1
            for v in (_mask((0, 1)), _mask((2, 3)), _mask((0, 7))):
                if sm[s] & v:
                    assert s in lists[v, :lens[v]], (s, v)
    assert straddling > 0, "no stage straddles two two-chunk classes: %s" % [m[0] for m in model]
    lonely = np.flatnonzero((np.abs(E) > 0).sum(1) == 1)
    assert lonely.size == 300 and np.all((on[2][lonely] & 0x7F) == _lib.PATH_EXACT), np.unique(on[2][lonely])


def test_a_whole_segment_disjoint_from_a_block(ctx, oracle):
    """20 013 targets, several segments under FORCE: 12 013 rows on {0,1} come first in the scan order, 8 000 on {2,3}
    after them, so the first segment holds {0,1} rows only and a {2,3} block's work item there walks stage 0 alone.
    Its queries' lists are full all the same, and every query keeps its path code."""
    E = _classes(np.random.default_rng(2602), (((0, 1), 12013), ((2, 3), 8000)))
    on, off, model, _ = skip_check(ctx, oracle, E, 0, E.shape[0], 0, "segments")
    tr = on[3]
    firsts = [t[0] for t in on[5]]
    assert tr["pass_segments"] > 1 and firsts[1] <= 12013 - 255, (tr, firsts)  # (segment 0: {0,1} rows only)
    assert on[5][0][1][_mask((2, 3))] == 1 and on[5][0][1][_mask((0, 1))] == model[0][0].size, on[5][0][1]
    assert np.array_equal(on[2], off[2]), "path codes change with the switch: %s" % np.flatnonzero(on[2] != off[2])[:8]
    q23 = np.flatnonzero(LR.chunk_masks(E) == _mask((2, 3)))
    assert np.all(on[4][q23] != KEY_INF), "a {2,3} query's list is not full"


def test_lists_that_only_the_first_stages_fill(ctx, oracle):
    """The kept stage 0 on its own: 20 lonely rows on chunk 4 as a rank-form query block against themselves and
    20 013 rows on {0,1} and {2,3}, several segments.  No target but the 20 shares a chunk with the block, and those
    sort first, into stage 0 of segment 0: the block's work item walks stage 0 of every segment and nothing else.  A
    query has at most two rows at similarity 1, so its K' candidates are d~ = 1 entries out of the first stages alone:
    every merged list must be full (no empty key) and hold the d~ patterns of the full scan (skip_check)."""
    rng = np.random.default_rng(2606)
    E = np.concatenate([_lonely_rows(20), _classes(rng, (((0, 1), 12013), ((2, 3), 8000)))])
    on, off, model, Q = skip_check(ctx, oracle, E, 0, 20, 1 << 20, "first-stages")
    tr = on[3]
    assert LR.block_masks(Q).tolist() == [16] and tr["pass_segments"] > 1, (LR.block_masks(Q), tr)
    for g, ((_, lens, lists), (sm, _, _)) in enumerate(zip(on[5], model)):
        assert lens[16] == 1 and lists[16, 0] == 0 and sm.size > 1 and (g > 0 or sm[0] & 16), (g, lens[16], sm[:2])
    assert tr["skip_stages_walked"] == tr["pass_segments"], tr
    assert np.all(on[4] != KEY_INF) and np.all(off[4] != KEY_INF), "a lonely query's list is not full"
    one = np.float32(1.0).view(np.uint32)
    assert np.all(((on[4] >> np.uint64(32)) == one).sum(1) >= on[3]["kp"] - 4), "lists not filled at d~ = 1"


def test_partial_ends_and_rank_form_blocks(ctx, oracle):
    """nt = 6 189 and 6 253: no multiples of 32, and 64 rows apart, so that one of them ends on a stage of one pair of
    tiles; then rank-form query blocks of 1, 33 and 257 rows with their own order table and row numbers from 2^20."""
    one_pair = 0
    for nt in (6189, 6253):
        E = _classes(np.random.default_rng(2603), (((0, 7), nt - 3000), ((1, 2, 3), 3000)))
        dev = _device_rows(ctx, E)
        on, _, _, _ = skip_check(ctx, oracle, E, 0, nt, 0, "partial/nt%d" % nt, dev=dev)
        firsts = [t[0] for t in on[5]] + [nt]
        tiles = [-(-(e - b) // 32) for b, e in zip(firsts, firsts[1:])]
        one_pair += any(t % 4 in (1, 2) for t in tiles)
        for q0, nq in ((0, 1), (5000, 33), (nt - 257, 257)):
            skip_check(ctx, oracle, E, q0, nq, 1 << 20, "partial/nt%d/block%d+%d" % (nt, q0, nq), dev=dev)
    assert one_pair > 0, "no segment ended on a stage of one pair of tiles"


def test_zero_query_block(ctx, oracle):
    """300 all-zero rows: the first query block of the scan order has mask 0 -- it walks stage 0 of every segment and
    nothing else -- and the zero rows get the closed-form answer."""
    E = _classes(np.random.default_rng(2604), (((1, 6), 1500), ((0, 2, 5), 1300)), zeros=300)
    on, _, model, Q = skip_check(ctx, oracle, E, 0, E.shape[0], 0, "zeros")
    assert LR.block_masks(Q)[0] == 0
    for (_, lens, _), (sm, _, _) in zip(on[5], model):
        assert lens[0] == 1 and sm.size > 1, (lens[0], sm.size)
    zero = np.flatnonzero(np.abs(E).sum(1) == 0)
    assert np.all((on[2][zero] & 0x7F) == _lib.PATH_ZERO) and on[3]["zero_queries"] == 300, on[3]


def test_nothing_to_skip(ctx, oracle):
    """dense signed rows on all eight chunks: no stage is left out, and the lists are those of the switch off"""
    E = _adversarial_rows("dense", 3000, D, np.random.default_rng(2605))
    on, _, _, _ = skip_check(ctx, oracle, E, 0, 3000, 0, "dense")
    assert on[3]["skip_stages_skipped"] == 0, on[3]
