"""The end of the live-chunk candidate pass (fdr_set_pass_tail; launch_rounds, PrefilterCall::pass_live and the query
selections of knn_merge_keys_kernel / knn_rerank_kernel): the groups issued in descending cost, and the merge + re-rank
of every group but the last queued on a further stream under the pass.  d = 128, k = 20, prefilter mode, the
duplicate-row layer off, live chunks forced (one case: AUTO at the size of rounds on two queues), the guarded and
poisoned workspace of tests/_guarded.py.

Every case runs the call with the switch off and with "auto", "order", "early" and "early_group", and checks (tail_check):
  * indices and distance bits of every mode against the switch off, bit for bit, and against the CPU oracle;
  * the captured candidate keys against the switch off (same_lists of tests/test_gpu_live_skip.py);
  * equal uncertified, range and zero counts, equal path codes per query, equal work items per instance;
  * the trace's group order -- ascending NL with the switch off, the reverse otherwise -- and the number of queries
    re-ranked before the join against the count made here from the device rows' block masks: 0 for "off" and "order";
    every query outside the group issued last for the early modes (forced calls run one launch per group on one queue,
    where both triggers coincide).
"""
import numpy as np
import pytest

import _live_rows as LR
from _guarded import knn_dev_guarded
from fedrann_amd import _lib
from test_gpu_candidates import CAPTURE
from test_gpu_live_chunks import _device_rows, _oracle_rows, _rounds_rows, same_bits
from test_gpu_live_skip import same_lists
from test_gpu_parity import _adversarial_rows

pytestmark = pytest.mark.gpu

K = 20
D = LR.D
MODES = ("auto", "order", "early", "early_group")
ALL8 = tuple(range(8))


def _call(ctx, Ehat, zero, q0, nq, t_base, tail, live="force"):
    """fdr_knn_dev of rows [q0, q0 + nq) against all rows with the switch at `tail`: (idx, dist, paths, trace, keys)"""
    import torch
    ctx.set_knn_mode("prefilter")
    ctx.set_dedup_mode("off")
    ctx.set_live_chunks(live)
    ctx.set_pass_tail(tail)
    ctx.set_knn_capture(CAPTURE)
    try:
        idx, dst, ws = knn_dev_guarded(ctx, Ehat, zero, q0, nq, t_base, D, K)
        paths = ctx.last_query_paths(nq)
        tr = ctx.last_knn_trace()
        assert tr["kind"] == "prefilter" and tr["pass_live"] == 1, tr
        del ws
        torch.cuda.empty_cache()
        keys, _ = ctx.last_candidates(nq, tr["kp"])
    finally:
        ctx.set_knn_capture(0)
        ctx.set_pass_tail("auto")
        ctx.set_live_chunks("auto")
        ctx.set_dedup_mode("auto")
        ctx.set_knn_mode("auto")
    return idx.cpu().numpy(), dst.cpu().numpy(), paths, tr, keys


def _order(tr):
    """the trace's groups in issue order: NL = 2 .. 6, 8 = the dense group"""
    v, out = tr["pass_group_order"], []
    while v:
        out.append(v & 15)
        v >>= 4
    return out


def _groups(tr):
    """ascending NL of the groups that ran, from the trace's work items"""
    g = [nl for nl in range(2, 7) if tr["pass_live_items_%d" % nl] > 0]
    return g + ([8] if tr["pass_live_dense_items"] > 0 else [])


def _queries_by_nl(Q):
    """queries per instance, from the device query rows' block masks (forced calls: no group joins another)"""
    nl = np.maximum(LR.expected_blocks(Q), 2)
    nl[nl > 6] = 8
    sizes = np.full(nl.size, 256)
    sizes[-1] = Q.shape[0] - 256 * (nl.size - 1)
    return {int(v): int(sizes[nl == v].sum()) for v in np.unique(nl)}


def tail_check(ctx, oracle, E, q0, nq, t_base, tag, dev=None, live="force", want_rows=None):
    """Every check of the module's docstring; returns ({mode: call}, device query rows)."""
    Ehat, zero = dev if dev is not None else _device_rows(ctx, E)
    off = _call(ctx, Ehat, zero, q0, nq, t_base, "off", live)
    rows = np.arange(nq) if want_rows is None else want_rows
    want = _oracle_rows(oracle, E, q0 + rows, K, t_base)
    assert same_bits((off[0][rows], off[1][rows]), want), "%s: the pass with the switch off differs from the oracle" % tag
    Q = Ehat[q0:q0 + nq].cpu().numpy()
    zq = zero.cpu().numpy()[q0:q0 + nq] != 0
    tro = off[3]
    asc = _groups(tro)
    assert _order(tro) == asc and tro["rerank_early_queries"] == 0, (tag, tro)
    by_nl = _queries_by_nl(Q) if live == "force" else None
    if by_nl is not None:
        assert sorted(by_nl) == asc and sum(by_nl.values()) == nq, (tag, by_nl, asc)
    runs = {"off": off}
    for mode in MODES:
        on = runs[mode] = _call(ctx, Ehat, zero, q0, nq, t_base, mode, live)
        tr = on[3]
        assert np.array_equal(on[0], off[0]), "%s/%s: indices change with the switch, first query %d" % (
            tag, mode, np.flatnonzero((on[0] != off[0]).any(1))[0])
        assert np.array_equal(on[1].view(np.uint32), off[1].view(np.uint32)), "%s/%s: distance bits change" % (tag, mode)
        assert same_bits((on[0][rows], on[1][rows]), want), "%s/%s differs from the oracle" % (tag, mode)
        same_lists(on[4], off[4], zq, "%s/%s" % (tag, mode))
        assert np.array_equal(on[2], off[2]), "%s/%s: path codes change: %s" % (tag, mode, np.flatnonzero(on[2] != off[2])[:8])
        for key in ("uncertified", "range_queries", "zero_queries", "pass_segments", "pass_launches", "pass_queues",
                    "pass_live_dense_items") + tuple("pass_live_items_%d" % n for n in range(2, 7)):
            assert tr[key] == tro[key], (tag, mode, key, tr[key], tro[key])
        print("%s/%s: order %s, %d of %d queries re-ranked before the join" % (
            tag, mode, _order(tr), tr["rerank_early_queries"], nq))
        if mode == "auto":  # (whichever parts AUTO takes: never the ascending order with early work)
            assert _order(tr) in (asc, asc[::-1]) and (tr["rerank_early_queries"] == 0 or _order(tr) == asc[::-1]), (tag, tr)
            continue
        assert _order(tr) == asc[::-1], (tag, mode, _order(tr), asc)
        if mode == "order":
            assert tr["rerank_early_queries"] == 0, (tag, mode, tr)
        elif by_nl is not None:  # everybody outside the group issued last: the smallest NL
            assert tr["rerank_early_queries"] == nq - by_nl[asc[0]], (tag, mode, tr["rerank_early_queries"], by_nl)
    return runs, Q


def _classes(rng, spec, zeros=0, shuffle=True):
    parts = [LR.signed_rows_of(ch, n, rng) for ch, n in spec]
    if zeros:
        parts.append(np.zeros((zeros, D), dtype=np.float32))
    E = np.concatenate(parts)
    if shuffle:
        E = E[rng.permutation(E.shape[0])]
    return np.ascontiguousarray(E)


# five NL groups and a dense one; 20 013 rows (five segments under FORCE), no multiple of 256
MIXED = (((1, 6), 3500), ((0, 2, 5), 3400), ((2, 3, 5, 7), 3300), ((0, 1, 3, 6, 7), 3200), ((0, 1, 2, 3, 5, 7), 3100),
         (ALL8, 3473))


@pytest.fixture(scope="module")
def mixed(ctx):
    E = _classes(np.random.default_rng(3601), MIXED, zeros=40)
    assert E.shape[0] == 20013
    return E, _device_rows(ctx, E)


def test_every_group_several_segments_short_last_block(ctx, oracle, mixed):
    """20 013 rows on classes of 2 .. 6 and 8 chunks and 40 zero rows, all-pairs: six groups, several segments; the
    last block of the scan order is short (20 013 = 78 x 256 + 45) and lies in the dense group, which the descending
    order issues FIRST and the early modes re-rank first.  The zero rows lie in the first block, in the group issued
    last: they get the closed-form answer behind the join."""
    E, dev = mixed
    runs, Q = tail_check(ctx, oracle, E, 0, E.shape[0], 0, "mixed", dev=dev)
    tr = runs["early"][3]
    assert tr["pass_segments"] > 1 and _order(tr) == [8, 6, 5, 4, 3, 2], tr
    assert LR.expected_blocks(Q)[-1] >= 7 and E.shape[0] % 256 != 0
    zero = np.flatnonzero(np.abs(E).sum(1) == 0)
    for mode, r in runs.items():
        assert np.all((r[2][zero] & 0x7F) == _lib.PATH_ZERO) and r[3]["zero_queries"] == 40, (mode, r[3])


def test_query_range_with_row_base(ctx, oracle, mixed):
    """rank form: rows [3 001, 3 001 + 1 333) of the same set as queries with an order table of their own, row numbers
    from 2^20; 1 333 is no multiple of 256"""
    E, dev = mixed
    runs, _ = tail_check(ctx, oracle, E, 3001, 1333, 1 << 20, "mixed/range", dev=dev)
    assert len(_order(runs["early"][3])) > 1 and runs["early"][3]["rerank_early_queries"] > 0, runs["early"][3]


def test_only_the_dense_group(ctx, oracle):
    """dense signed rows on all eight chunks: one group, nothing before the join, and the trace says so"""
    E = _adversarial_rows("dense", 3000, D, np.random.default_rng(3602))
    runs, _ = tail_check(ctx, oracle, E, 0, 3000, 0, "dense-only")
    for mode, r in runs.items():
        assert _order(r[3]) == [8] and r[3]["rerank_early_queries"] == 0, (mode, r[3])


def test_no_dense_group_and_zero_rows_in_an_early_group(ctx, oracle):
    """No block of seven or eight chunks.  The 10 zero rows sort first and share block 0 with 100 rows on {0,1} and the
    first rows on {2,3}: a block of FOUR live chunks, while the blocks behind it hold {2,3} rows alone -- so the zero
    rows' block lies in the NL = 4 group, which is issued (and, in the early modes, re-ranked) before the NL = 2 group:
    the zero rows are listed by an early launch and still get the closed-form answer."""
    spec = (((0, 1), 100), ((2, 3), 1500), ((0, 2, 5), 1100), ((0, 1, 3, 4), 1390))
    E = _classes(np.random.default_rng(3603), spec, zeros=10)
    runs, Q = tail_check(ctx, oracle, E, 0, E.shape[0], 0, "no-dense")
    blocks = LR.expected_blocks(Q)
    assert blocks[0] == 4 and blocks[1] == 2 and blocks.max() <= 6, blocks
    tr = runs["early"][3]
    assert _order(tr)[-1] == 2 and 4 in _order(tr)[:-1] and tr["pass_live_dense_items"] == 0, tr
    zero = np.flatnonzero(np.abs(E).sum(1) == 0)
    for mode, r in runs.items():
        assert np.all((r[2][zero] & 0x7F) == _lib.PATH_ZERO) and r[3]["zero_queries"] == 10, (mode, r[3])


def test_zero_rows_in_the_dense_group(ctx, oracle):
    """300 rows on all eight chunks and 30 zero rows in front of them, then 2 700 rows more: block 0 -- zero rows and
    eight-chunk rows -- is dense, like every block: the zero rows' closed-form answer in the only (late) group"""
    E = _classes(np.random.default_rng(3604), ((ALL8, 3000),), zeros=30)
    runs, Q = tail_check(ctx, oracle, E, 0, E.shape[0], 0, "dense-zeros")
    assert LR.expected_blocks(Q)[0] == 8
    zero = np.flatnonzero(np.abs(E).sum(1) == 0)
    assert np.all((runs["early"][2][zero] & 0x7F) == _lib.PATH_ZERO)


def test_a_group_below_one_launch_joins_its_neighbour_on_two_queues(ctx, oracle):
    """AUTO at the size of rounds (1.15 x 512 x CUs rows: test_gpu_live_chunks._rounds_rows): launches of 512 work items
    dealt to two queues, and the three-chunk blocks -- fewer items than a launch -- join instance 4.  Here the two
    triggers differ, and the early work waits for events on both queues.  The oracle on a sample of the rows."""
    n = int(1.15 * 512 * ctx.device_info()["cus"])
    E = _rounds_rows(n, np.random.default_rng(3605))
    sample = np.unique(np.concatenate([np.random.default_rng(5).choice(n, 192, replace=False), [0, n - 1]]))
    runs, Q = tail_check(ctx, oracle, E, 0, n, 0, "rounds", live="auto", want_rows=sample)
    tr = runs["early_group"][3]
    assert tr["pass_queues"] == 2 and tr["pass_launches"] > 2, tr
    assert (LR.expected_blocks(Q) == 3).sum() > 0 and tr["pass_live_items_3"] == 0 and tr["pass_live_items_4"] > 0, tr
    for mode in ("early", "early_group"):
        assert 0 < runs[mode][3]["rerank_early_queries"] < n, (mode, runs[mode][3])
    # each group's own trigger leaves only the group issued last behind the join; the common one may leave more
    assert runs["early_group"][3]["rerank_early_queries"] >= runs["early"][3]["rerank_early_queries"]
