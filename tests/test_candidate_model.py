"""The float64 model and checker of tests/_candidate_model.py, on the CPU: it tells the faults apart that the GPU
tests (tests/test_gpu_candidates.py) are there to catch, and it rejects wrong candidate lists and range sets."""
import numpy as np
import pytest

import _candidate_model as M
import _live_rows as L
from test_gpu_parity import _adversarial_rows

KINDS = ("fp16_midpoints", "fp16_subnormals", "dense")


def _model_lists(model, qrows, kp, qbits):
    """Lists the way a faultless pass builds them: the kp targets of smallest d_model, keyed on the device's grid."""
    full = model.row_dists(qrows)
    order = np.argsort(full, axis=1, kind="stable")[:, :kp]
    q = M.qm1(qbits)
    d = np.take_along_axis(full, order, 1)
    dq = (np.float32(q) - np.rint((1 - d) * q).astype(np.float32)) / np.float32(q)
    keys = (dq.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        (order + model.t_base).astype(np.uint64)
    return keys, full, order


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [128, 256, 500])
def test_rounding_faults_are_visible_on_adversarial_rows(oracle, kind, d):
    """Round-toward-zero conversion moves the listed pairs' distances by far more than 4 tol on every set; flushing
    fp16 subnormals does so on the subnormal set (at d = 500 its largest effect, 1.2e-4, still exceeds tol 4x over on
    some pairs).  So the GPU tests' tol separates the kernels' RNE conversion from both faults."""
    rng = np.random.default_rng(d + len(kind))
    E = _adversarial_rows(kind, 1500, d, rng)
    Eh, _, zero = oracle.normalize(E)
    models = {f: M.Model(Eh, zero, d, flavour=f) for f in ("rne", "rtz", "ftz")}
    qrows = np.arange(0, 1500, 7)
    _, _, lists = _model_lists(models["rne"], qrows, 32, 20)
    tol = M.tolerance(d, 20)
    ref = models["rne"].pair_dists(qrows, lists, exact=False)[0]
    far = {f: np.abs(models[f].pair_dists(qrows, lists, exact=False)[0] - ref) for f in ("rtz", "ftz")}
    assert (far["rtz"] > 4 * tol).mean() > 0.1, (far["rtz"] > 4 * tol).mean()
    if kind == "fp16_subnormals":
        assert (far["ftz"] > (4 * tol if d <= 256 else tol)).mean() > 0.05, far["ftz"].max()


@pytest.fixture(scope="module")
def mid_set(oracle):
    rng = np.random.default_rng(31)
    E = _adversarial_rows("dense", 1200, 128, rng)
    Eh, _, zero = oracle.normalize(E)
    model = M.Model(Eh, zero, 128, t_base=1 << 20)
    qrows = np.arange(0, 1200, 5)
    keys, full, order = _model_lists(model, qrows, 32, 20)
    return model, qrows, keys, full, order


def test_model_lists_pass(mid_set):
    model, qrows, keys, _, _ = mid_set
    rep = M.check_lists(model, keys, 20, qrows, complete=np.arange(len(qrows)))
    assert rep["lists"] == len(qrows) and rep["max_err_model"] <= rep["tol"]
    assert rep["max_err_exact"] + 1e-6 < rep["eps"] and rep["completeness_min_gap"] >= 0


def test_checker_rejects_a_swapped_member(mid_set):
    """One member replaced by the target ranked K' + 3 (its key keeps the member's d~): accuracy and completeness both
    break -- the completeness check alone is asked to see it."""
    model, qrows, keys, full, _ = mid_set
    bad = keys.copy()
    i = 17
    far = np.argsort(full[i], kind="stable")[32 + 2]
    bad[i, 5] = (bad[i, 5] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(far + model.t_base)
    with pytest.raises(AssertionError, match="off the model"):
        M.check_lists(model, bad, 20, qrows)
    # the member ranked K' + 3 left out, its key in the list at its own place: only completeness can see it
    dq = bad[i, 5] >> np.uint64(32)
    cut = keys.copy()
    cut[i, 31] = (dq << np.uint64(32)) | np.uint64(far + model.t_base)
    gap = full[i][np.argsort(full[i], kind="stable")[31]] - full[i][far]
    if abs(gap) > 2 * M.tolerance(128, 20):
        with pytest.raises(AssertionError):
            M.check_lists(model, cut, 20, qrows, complete=[i])


def test_checker_rejects_a_moved_distance(mid_set):
    model, qrows, keys, _, _ = mid_set
    d, rows, _ = M.decode(keys)
    tol = M.tolerance(128, 20)
    bad = keys.copy()
    i = 40
    nd = np.float32(d[i, 31] + 2 * tol)  # (the last entry: the list stays ascending)
    bad[i, 31] = (np.uint64(nd.view(np.uint32)) << np.uint64(32)) | np.uint64(rows[i, 31])
    with pytest.raises(AssertionError, match="off the model"):
        M.check_lists(model, bad, 20, qrows)


def test_checker_rejects_a_duplicate_row(mid_set):
    model, qrows, keys, _, _ = mid_set
    bad = keys.copy()
    bad[3, 9] = (bad[3, 9] & np.uint64(0xFFFFFFFF00000000)) | (bad[3, 8] & np.uint64(0xFFFFFFFF))
    with pytest.raises(AssertionError, match="twice"):
        M.check_lists(model, bad, 20, qrows)


def test_checker_rejects_short_lists_and_foreign_rows(mid_set):
    model, qrows, keys, _, _ = mid_set
    bad = keys.copy()
    bad[0, 31] = M.KEY_INF
    with pytest.raises(AssertionError, match="valid keys"):
        M.check_lists(model, bad, 20, qrows)
    bad = keys.copy()
    bad[1, 31] = (bad[1, 31] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(model.t_base + model.nt)
    with pytest.raises(AssertionError, match="outside"):
        M.check_lists(model, bad, 20, qrows)


def test_range_checker(mid_set):
    """The model's own sets {d_model <= theta} pass; one row of A missing, a row twice or a row far above theta
    fails; an overflowed count is bracketed by |A| and |B|."""
    model, qrows, _, full, _ = mid_set
    qs = qrows[:12]
    theta = np.sort(full[:12], axis=1)[:, 60].astype(np.float32)
    counts = np.zeros(12, np.int32)
    rows = np.full((12, M.RANGE_CAP), -1, np.int32)
    for i in range(12):
        got = np.flatnonzero(full[i] <= theta[i]) + model.t_base
        counts[i] = got.size
        rows[i, :got.size] = got[::-1]
    rep = M.check_ranges(model, qs, theta, counts, rows, 20)
    assert rep["queries"] == 12 and rep["overflowed"] == 0
    tol = M.tolerance(128, 20)
    i = int(np.argmax([np.sum(full[j] <= theta[j] - tol) for j in range(12)]))
    A = np.flatnonzero(full[i] <= theta[i] - tol) + model.t_base
    assert A.size > 0
    miss_rows, miss_cnt = rows.copy(), counts.copy()
    keep = rows[i, :counts[i]][rows[i, :counts[i]] != A[0]]
    miss_rows[i] = -1
    miss_rows[i, :keep.size] = keep
    miss_cnt[i] = keep.size
    with pytest.raises(AssertionError, match="missed"):
        M.check_ranges(model, qs, theta, miss_cnt, miss_rows, 20)
    dup_rows, dup_cnt = rows.copy(), counts.copy()
    dup_rows[i, counts[i]] = rows[i, 0]
    dup_cnt[i] += 1
    with pytest.raises(AssertionError, match="twice"):
        M.check_ranges(model, qs, theta, dup_cnt, dup_rows, 20)
    far_rows, far_cnt = rows.copy(), counts.copy()
    far_rows[i, counts[i]] = int(np.argmax(full[i])) + model.t_base
    far_cnt[i] += 1
    with pytest.raises(AssertionError, match="above theta"):
        M.check_ranges(model, qs, theta, far_cnt, far_rows, 20)
    big = np.full(12, 2000, np.int32)  # (more than the model's sets hold: |B| < count)
    with pytest.raises(AssertionError, match="outside"):
        M.check_ranges(model, qs, theta, big, rows, 20)


# ---- the live-chunk pass (knn_prefilter_live_kernel<NL>): the GPU tests' inputs can see its faults -------------------
LIVE_FAULTS = ("drop", "swap", "neighbour")


def _emulate_live_pass(model, ids, kp, qbits, fault=None, nl=None):
    """The live-chunk pass over the model's fp16 rows [n, 128], every row a query: the rows in scan order, blocks of 256
    queries, block b multiplying only the chunks ids[b] (ascending ids; float64 sums), the kp targets of smallest
    d = 1 - clamp(s, 0, 1) keyed on the device's grid.  `fault`, applied to every block that runs as instance `nl`:
      "drop"       one chunk that is non-empty in the block is left out of its ids;
      "swap"       the two 8-component halves of one such chunk change places in the block's query fragments;
      "neighbour"  the block reads the next block's packed id word (the last block: the one before), nl nibbles of it
                   -- ids past the neighbour's own read as chunk 0, as the zero nibbles of the word would."""
    H = model.H.astype(np.float64)
    n = H.shape[0]
    order = L.scan_order(model.X)
    masks = L.block_masks(model.X)
    assert len(ids) == len(masks)
    keys = np.empty((n, kp), np.uint64)
    q = M.qm1(qbits)
    for b, own in enumerate(ids):
        rows = order[256 * b:256 * b + 256]
        Q, use = H[rows], list(own)
        if fault is not None and len(own) == nl:
            live = [c for c in own if (int(masks[b]) >> c) & 1]
            if fault == "drop":
                use.remove(live[0])
            elif fault == "swap":
                c = live[0]
                Q = Q.copy()
                Q[:, 16 * c:16 * c + 8], Q[:, 16 * c + 8:16 * c + 16] = H[rows, 16 * c + 8:16 * c + 16], H[rows, 16 * c:16 * c + 8]
            elif fault == "neighbour":
                other = ids[b + 1] if b + 1 < len(ids) else ids[b - 1]
                use = (list(other) + [0] * 8)[:nl]
            else:
                raise ValueError(fault)
        s = np.zeros((len(rows), n))
        for c in use:
            s += Q[:, 16 * c:16 * c + 16] @ H[:, 16 * c:16 * c + 16].T
        d = 1.0 - np.clip(s, 0.0, 1.0)
        top = np.argsort(d, axis=1, kind="stable")[:, :kp]
        dq = (np.float32(q) - np.rint((1 - np.take_along_axis(d, top, 1)) * q).astype(np.float32)) / np.float32(q)
        keys[rows] = (dq.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
            (top + model.t_base).astype(np.uint64)
    return keys


def _live_model(oracle, E, d):
    Eh, _, zero = oracle.normalize(E)
    X = np.zeros((E.shape[0], 128), np.float32)
    X[:, :Eh.shape[1]] = Eh
    return M.Model(X, zero, d)


def _faults_are_seen(model, ids, nls, faults, tag):
    n = model.nt
    keys = _emulate_live_pass(model, ids, 32, 20)
    rep = M.check_lists(model, keys, 20, np.arange(n), complete=np.arange(n))
    assert rep["lists"] == n - int(model.zero.sum()) and rep["completeness_min_gap"] >= 0, (tag, rep)
    for nl in nls:
        assert any(len(b) == nl for b in ids), (tag, nl, [len(b) for b in ids])
        for fault in faults:
            bad = _emulate_live_pass(model, ids, 32, 20, fault=fault, nl=nl)
            with pytest.raises(AssertionError):
                M.check_lists(model, bad, 20, np.arange(n), complete=np.arange(n))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [16, 32, 48, 64, 80, 96, 40, 100])
def test_live_chunk_faults_are_visible_on_dense_signed_rows(oracle, kind, d):
    """Set 1 of tests/test_gpu_live_chunks.py at 1 200 rows: every block holds all ceil(d / 16) chunks (one chunk: run
    as two, with a padded id; seven: the dense kernel, no live instance).  The fault-free emulation passes every check;
    a dropped chunk and swapped halves fail them.  Where every block carries the same ids, reading a neighbour's changes
    nothing (asserted: the emulation returns the same keys) -- that fault is set 2's to show."""
    rng = np.random.default_rng(d + 7 * len(kind))
    model = _live_model(oracle, _adversarial_rows(kind, 1200, d, rng), d)
    ids = L.block_ids(model.X)
    nch = -(-d // 16)
    want = list(range(8)) if nch >= 7 else list(range(max(nch, 2)))
    # (the sparse kinds' first block, the rows of fewest chunks, may lack a chunk where the last one is half full)
    assert ids[-1] == want and (kind != "dense" or all(b == want for b in ids)), (ids, want)
    if nch >= 7:
        _faults_are_seen(model, ids, (), (), "%s-%d" % (kind, d))
        return
    _faults_are_seen(model, ids, (len(want),), ("drop", "swap"), "%s-%d" % (kind, d))
    if all(b == want for b in ids):
        same = _emulate_live_pass(model, ids, 32, 20, fault="neighbour", nl=len(want))
        assert np.array_equal(same, _emulate_live_pass(model, ids, 32, 20))


def test_live_chunk_faults_are_visible_on_signed_mask_classes(oracle):
    """Set 2 at 2 000 rows, the class sizes chosen so that its eight blocks run as 3, 2, 3, 5, 4, 5, dense and 6 (the
    first holds the zero rows, the lonely rows and the start of the two-chunk class; two straddle a class boundary):
    every instance NL = 2 .. 6 has a block, and each of the three faults on each NL fails a check."""
    rng = np.random.default_rng(2208)
    E, _ = L.signed_classes(rng, sizes=(402, 300, 468, 300, 420), lonely=100, zeros=10)
    assert E.shape[0] == 2000
    model = _live_model(oracle, E, 128)
    ids = L.block_ids(model.X)
    assert [len(b) for b in ids] == [3, 2, 3, 5, 4, 5, 8, 6], ids
    _faults_are_seen(model, ids, (2, 3, 4, 5, 6), LIVE_FAULTS, "signed classes")


def test_rounding_helpers():
    x = np.array([1 + 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 3e-6, -3e-6, 2.0 ** -25 * 1.5], np.float32)
    assert np.array_equal(M.to_half(x, "rne"), np.array([1, -(1 + 4 * 2.0 ** -11), 2.98023224e-06, -2.98023224e-06,
                                                          2.0 ** -24], np.float32))
    assert np.array_equal(M.to_half(x, "rtz")[:2], np.array([1, -(1 + 2 * 2.0 ** -11)], np.float32))
    assert np.all(np.abs(M.to_half(x, "rtz")) <= np.abs(x))
    assert np.array_equal(M.to_half(x, "ftz")[2:], np.zeros(3, np.float32))
    assert abs(M.prefilter_eps(20) - (0.00105 + 0.5 / (2 ** 20 - 2) + 1e-6)) < 1e-9
