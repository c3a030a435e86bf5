"""The float64 model and checker of tests/_candidate_model.py, on the CPU: it tells the faults apart that the GPU
tests (tests/test_gpu_candidates.py) are there to catch, and it rejects wrong candidate lists and range sets."""
import numpy as np
import pytest

import _candidate_model as M
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


def test_rounding_helpers():
    x = np.array([1 + 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 3e-6, -3e-6, 2.0 ** -25 * 1.5], np.float32)
    assert np.array_equal(M.to_half(x, "rne"), np.array([1, -(1 + 4 * 2.0 ** -11), 2.98023224e-06, -2.98023224e-06,
                                                          2.0 ** -24], np.float32))
    assert np.array_equal(M.to_half(x, "rtz")[:2], np.array([1, -(1 + 2 * 2.0 ** -11)], np.float32))
    assert np.all(np.abs(M.to_half(x, "rtz")) <= np.abs(x))
    assert np.array_equal(M.to_half(x, "ftz")[2:], np.zeros(3, np.float32))
    assert abs(M.prefilter_eps(20) - (0.00105 + 0.5 / (2 ** 20 - 2) + 1e-6)) < 1e-9
