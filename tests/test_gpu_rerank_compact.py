"""Re-rank from compact rows (to_half_compact_kernel and the compact route of knn_rerank_kernel,
fedrann_amd/csrc/knn_prefilter.inc): at d <= 128 a needed candidate is re-ranked from its row's record of non-zero
components, a row with more non-zeros than a record holds from its whole fp32 row.  Prefilter mode, the duplicate-row
layer off, workspace and outputs poisoned between canaries (tests/_guarded.py).

Rows (_rows).  Every row holds a common pair of heavy components (0 and 1, value 1), so every row is similar to every
other.  Rows are assigned in rotation to classes of NNZ non-zeros: the record's edges -+ 1 and dense rows.  A row of
three or more non-zeros also holds a tag component (value 0.5) it shares with the rows of its group, a run of
consecutive rows sized so that a group's tagged rows number between k and K': a tagged query's K nearest rows are its
group (distance ~ 1e-3 and below), the K'-th candidate lies outside it (distance >= 0.05), so the certificate holds
and the needed candidates are the group's rows -- all classes of the rotation but 1 and 2, hence both halves of a
record and the dense route for every such query (asserted on the oracle's neighbours).  The remaining non-zeros are
small unique extras (2e-3 .. 6e-3, signed) on random other components, so that no two tagged rows are equal and their
similarities are distinct.  Rows of one or two non-zeros cannot hold a tag: the one-component rows are equal after
normalisation and the two-component rows lie within 1e-3 of one another, so both kinds sit on plateaus wider than K'
and take the range pass (they are candidates of nobody's group).  Some rows get explicit -0.0f components (zeros to the
record) and a handful of all-zero rows is appended.

Every case checks (compact_check): indices and distance bits against the CPU oracle with the switch on and off,
equal path codes, the trace's switch, and its long-row count against numpy's count of the device rows' non-zeros.
"On" is FORCE: three classes in ten are long here, and AUTO reads the records only while at most one row in
LONG_SHARE is long (test_auto_reads_the_records_only_while_few_rows_are_long).
"""
import numpy as np
import pytest

from _guarded import knn_dev_guarded
from fedrann_amd import _lib
from test_gpu_live_chunks import _device_rows, _oracle_rows, same_bits

pytestmark = pytest.mark.gpu

HALF, ENTRIES = 12, 24  # entries of a record's half and of a record (knn_workspace.inc: RC_HALF_ENTRIES, RC_ENTRIES)
SERVED_DP = 128         # the width the records serve (RC_DP)
LONG_SHARE = 32         # AUTO reads the records while long rows * LONG_SHARE <= target rows (RC_LONG_SHARE)
NZEROS = 5


def _classes(d):
    """non-zeros per row: 1, 2, the edges of a record's halves -+ 1, beyond a record, dense"""
    return (1, 2, HALF - 1, HALF, HALF + 1, ENTRIES - 1, ENTRIES, ENTRIES + 1, 40, d)


def _kp(k):
    return (k + (12 if k + 12 <= (32 if k + 8 <= 32 else 64) else 8) + 1) & ~1  # (knn_plan.inc: prefilter_extra)


def _rows(n, d, k, classes, seed):
    """n rows of the module docstring's construction and NZEROS all-zero rows, float32 [n + NZEROS, d]"""
    rng = np.random.default_rng(seed)
    tagged = sum(c >= 3 for c in classes) / len(classes)
    per_group = int(np.ceil((k + _kp(k)) / 2 / tagged))  # rows of a group: its tagged rows number ~ (k + K') / 2
    assert 2 + -(-n // per_group) <= d, "more groups than tag components"
    E = np.zeros((n + NZEROS, d), dtype=np.float32)
    for i in range(n):
        m = classes[i % len(classes)]
        E[i, 0] = 1.0
        if m >= 2:
            E[i, 1] = 1.0 + (1e-3 * rng.random() if m == 2 else 0.0)  # (two-component rows: distinct directions)
        if m >= 3:
            tag = 2 + i // per_group
            E[i, tag] = 0.5
            free = np.setdiff1d(np.arange(2, d), [tag])
            where = rng.choice(free, m - 3, replace=False)
            E[i, where] = rng.uniform(2e-3, 6e-3, m - 3) * rng.choice([-1.0, 1.0], m - 3)
        if i % 7 == 3 and m < d:  # explicit -0.0f on some of the row's zero components
            zeros = np.flatnonzero(E[i] == 0)
            E[i, rng.choice(zeros, min(3, zeros.size), replace=False)] = -0.0
    assert np.signbit(E[E == 0]).any()
    return E


def _call(ctx, Ehat, zero, q0, nq, t_base, d, k, mode):
    ctx.set_knn_mode("prefilter")
    ctx.set_dedup_mode("off")
    ctx.set_rerank_compact(mode)
    try:
        idx, dst, ws = knn_dev_guarded(ctx, Ehat, zero, q0, nq, t_base, d, k)
        paths = ctx.last_query_paths(nq)
        tr = ctx.last_knn_trace()
        del ws
    finally:
        ctx.set_rerank_compact("auto")
        ctx.set_dedup_mode("auto")
        ctx.set_knn_mode("auto")
    assert tr["kind"] == "prefilter", tr
    return idx.cpu().numpy(), dst.cpu().numpy(), paths, tr


def compact_check(ctx, oracle, E, q0, nq, t_base, k, tag, served=True, mixed=True, mode="force"):
    d = E.shape[1]
    Ehat, zero = _device_rows(ctx, E)
    on = _call(ctx, Ehat, zero, q0, nq, t_base, d, k, mode)
    off = _call(ctx, Ehat, zero, q0, nq, t_base, d, k, "off")
    want = _oracle_rows(oracle, E, q0 + np.arange(nq), k, t_base)
    assert same_bits(on[:2], want), "%s: the compact re-rank differs from the oracle" % tag
    assert same_bits(off[:2], want), "%s: the dense re-rank (switch off) differs from the oracle" % tag
    assert same_bits(on[:2], off[:2]), tag
    assert np.array_equal(on[2], off[2]), "%s: path codes change with the switch: %s" % (tag, np.flatnonzero(on[2] != off[2])[:8])
    nnz = ((Ehat.cpu().numpy().view(np.uint32) & 0x7FFFFFFF) != 0).sum(1)  # of the device rows, all targets
    n_long = int((nnz > ENTRIES).sum())
    tr, tro = on[3], off[3]
    certified = (on[2] & 0x7F) == _lib.PATH_CERTIFIED
    print("%s: %d queries, %d certified; long rows %d (numpy %d), trace on %d / off %d" % (
        tag, nq, certified.sum(), tr["rerank_compact_long"], n_long, tr["rerank_compact"], tro["rerank_compact"]))
    assert (tro["rerank_compact"], tro["rerank_compact_entries"], tro["rerank_compact_long"]) == (0, 0, 0), (tag, tro)
    if not served:
        assert (tr["rerank_compact"], tr["rerank_compact_entries"], tr["rerank_compact_long"]) == (0, 0, 0), (tag, tr)
        return on
    kept = mode == "force" or n_long * LONG_SHARE <= E.shape[0]
    assert tr["rerank_compact"] == kept and tr["rerank_compact_entries"] == ENTRIES, (tag, tr)
    assert tr["rerank_compact_long"] == n_long and n_long > 0, (tag, tr["rerank_compact_long"], n_long)
    # the certified queries are the ones the kernel re-ranks: most of the tagged rows, and their neighbours mix routes
    assert certified.sum() >= nq // 2, (tag, int(certified.sum()), nq)
    if mixed:
        nb = nnz[want[0][certified] - t_base]
        routes = (nb <= HALF).any(1) & ((nb > HALF) & (nb <= ENTRIES)).any(1) & (nb > ENTRIES).any(1)
        assert routes.sum() >= 0.9 * certified.sum(), (tag, int(routes.sum()), int(certified.sum()))
    return on


def test_one_batch_d128_k20(ctx, oracle):
    """K' = 32: the candidates sit in the first half-wave"""
    E = _rows(2500, 128, 20, _classes(128), 3201)
    compact_check(ctx, oracle, E, 0, E.shape[0], 0, 20, "d128/k20")


def test_two_batches_d128_k50(ctx, oracle):
    """K' = 62: candidates on all 64 lanes, several dense batches"""
    E = _rows(2500, 128, 50, _classes(128), 3202)
    compact_check(ctx, oracle, E, 0, E.shape[0], 0, 50, "d128/k50")


def test_wider_rows_keep_the_dense_route(ctx, oracle):
    """d = 256 is not served: no records, the trace says so, and the results are the oracle's either way"""
    E = _rows(2000, 256, 20, _classes(256), 3203)
    compact_check(ctx, oracle, E, 0, E.shape[0], 0, 20, "d256/k20", served=False)


def test_narrower_rows_padded_to_the_served_width(ctx, oracle):
    """d = 100 pads to 128 components: served, with the padding as zeros of every row"""
    assert ctx.padded_dim(100) == SERVED_DP
    E = _rows(2000, 100, 20, _classes(100), 3204)
    compact_check(ctx, oracle, E, 0, E.shape[0], 0, 20, "d100/k20")


def test_query_block_with_a_target_base(ctx, oracle):
    """a rank-form call: queries [700, 1601) of the rows, row numbers from 2^20 + 5"""
    E = _rows(2500, 128, 20, _classes(128), 3205)
    compact_check(ctx, oracle, E, 700, 901, (1 << 20) + 5, 20, "d128/k20/block")


def test_every_row_long(ctx, oracle):
    """rows of ENTRIES + 1, 40 and 128 non-zeros only: the route is on and every candidate goes dense"""
    E = _rows(2000, 128, 20, (ENTRIES + 1, 40, 128), 3206)
    on = compact_check(ctx, oracle, E, 0, E.shape[0], 0, 20, "d128/k20/long", mixed=False)
    assert on[3]["rerank_compact_long"] == 2000, on[3]


def test_auto_reads_the_records_only_while_few_rows_are_long(ctx, oracle):
    """AUTO: one long row in 80 keeps the route on; the other tests' three in ten build the records, count the long rows
    and leave every candidate to the dense route.  The same results either way."""
    few = (HALF - 1, HALF, HALF + 1, ENTRIES - 1, ENTRIES, HALF, HALF + 1, ENTRIES - 1) * 10
    few = few[:-1] + (ENTRIES + 1,)
    E = _rows(2500, 128, 20, few, 3207)
    on = compact_check(ctx, oracle, E, 0, E.shape[0], 0, 20, "d128/k20/auto-few", mixed=False, mode="auto")
    assert on[3]["rerank_compact"] == 1 and 0 < on[3]["rerank_compact_long"] * LONG_SHARE <= E.shape[0], on[3]
    E = _rows(2500, 128, 20, _classes(128), 3208)
    on = compact_check(ctx, oracle, E, 0, E.shape[0], 0, 20, "d128/k20/auto-many", mixed=False, mode="auto")
    assert on[3]["rerank_compact"] == 0 and on[3]["rerank_compact_long"] * LONG_SHARE > E.shape[0], on[3]
