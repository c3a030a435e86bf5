"""A plain float64 model of the prefilter mode's fp16 candidate pass and range pass, and the checks of what the device
captured (fdr_set_knn_capture) against it.  Numpy only; the GPU tests feed it the device's own normalised rows.

The model.  The pass converts the normalised fp32 rows x^ (fdr_normalize_dev) to fp16 with round-to-nearest-even,
subnormals kept (to_half_kernel / to_half_ordered_kernel), multiplies them on the fp16 MFMA with fp32 accumulation, and
keys d~ = qd / QM1, qd = QM1 - rint(clamp(s~, 0, 1) * QM1), QM1 = 2^qbits - 2 (knn_prefilter.inc).  The model rounds
x^ the same way (numpy's float16 cast is RNE with subnormals), forms s = x_h . y_h in float64 (the products of two fp16
numbers are exact, the float64 sum is within d 2^-53 of the real one) and d_model = 1 - clamp(s, 0, 1).

The tolerance |d~ - d_model| <= tol(d, qbits) = d 2^-24 (1 + 2^-10) + 0.5 / QM1 + 2^-23:
  - fp32 accumulation of at most d non-zero products (the padding adds exact zeros): at most d roundings of relative
    size 2^-24, each on a partial sum bounded by sum |x_h||y_h| <= |x_h| |y_h| <= (1 + 2^-11)^2 <= 1 + 2^-10 (each
    component grows by at most half an fp16 ulp, 2^-11 relative; |x^| = 1 to fp32 precision) -- the gamma_d factor
    1 / (1 - d 2^-24) adds under 1e-9 and is covered by the last term;
  - the key grid: rint moves sc * QM1 by at most 1/2 step, 0.5 / QM1 in distance;
  - the fp32 product sc * QM1 and the quotient qd / QM1: one rounding each, 2^-24 apiece in distance (2^-23).
clamp() is 1-Lipschitz, so the bound on the similarity carries over to the distance.  The range pass compares the
unquantised fp32 distance 1 - clamp(s~) against theta, so the same tol (its grid term to spare) bounds it as well.

The certificate premise (knn_plan.inc prefilter_eps, knn_prefilter.inc:1-21): |d~ - d_exact| + 1e-6 <= eps(qbits),
d_exact the float64 distance of the fp32 rows (the canonical fp32 chain lies within 1e-6 of it)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

KEY_INF = np.uint64(0xFFFFFFFFFFFFFFFF)
RANGE_CAP = 1024
RANGE_SLACK = 3.0e-7       # the range kernels' sfloor slack (knn_prefilter.inc knn_range_kernel)
PREFILTER_EPS = 0.00105    # FDR_PREFILTER_EPS (knn_plan.inc)
THREADS = min(16, os.cpu_count() or 1)
CHUNK_BYTES = 64 << 20     # float64 gathered per work item (THREADS of them in flight: ~1 GB)


def qm1(qbits):
    return (1 << qbits) - 2


def tolerance(d, qbits):
    return d * 2.0 ** -24 * (1 + 2.0 ** -10) + 0.5 / qm1(qbits) + 2.0 ** -23


def prefilter_eps(qbits):
    """prefilter_eps() of knn_plan.inc, in the same fp32 arithmetic (qbits = min(20, 32 - ib))."""
    f = np.float32
    return float(f(f(PREFILTER_EPS) + f(0.5) / f(qm1(qbits))) + f(1.0e-6))


def to_half(X, flavour="rne"):
    """fp32 -> fp16 values (as float32, exactly): "rne" round to nearest even with subnormals (what the kernels must
    do); "rtz" round toward zero; "ftz" RNE with the subnormal results flushed to zero (the two faults the GPU tests
    are built to see)."""
    X = np.asarray(X, dtype=np.float32)
    h = X.astype(np.float16)
    if flavour == "rtz":
        over = np.abs(h.astype(np.float32)) > np.abs(X)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    elif flavour == "ftz":
        h = np.where(np.abs(h) < np.float16(2.0 ** -14), np.float16(0), h)
    elif flavour != "rne":
        raise ValueError(flavour)
    return h.astype(np.float32)


def _parallel(fn, items):
    if len(items) <= 1 or THREADS <= 1:
        return [fn(it) for it in items]
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, items))


class Model:
    """The targets T (rows of the device's Ehat, any component order: both sides share it), global row numbers from
    t_base.  Query rows are named by their row in T (the tests' queries are always a block of the targets)."""

    def __init__(self, Ehat, zero, d, t_base=0, flavour="rne"):
        self.X = np.ascontiguousarray(Ehat, dtype=np.float32)
        self.H = to_half(self.X, flavour)
        self.zero = np.asarray(zero).astype(bool)
        self.d, self.t_base, self.nt = int(d), int(t_base), self.X.shape[0]

    @staticmethod
    def _dist(s):
        return 1.0 - np.clip(s, 0.0, 1.0)

    def pair_dists(self, qrows, trows, exact=True):
        """d_model (and d_exact) [len(qrows), m] of query row qrows[i] against T rows trows[i, :] (local)."""
        qrows = np.asarray(qrows, np.int64)
        trows = np.asarray(trows, np.int64)
        m, dp = trows.shape[1], self.X.shape[1]
        step = max(1, CHUNK_BYTES // max(1, m * dp * 8))
        out_m = np.empty(trows.shape, np.float64)
        out_e = np.empty(trows.shape, np.float64) if exact else None

        def work(lo):
            hi = min(lo + step, len(qrows))
            for src, out in ((self.H, out_m), (self.X, out_e)):
                if out is None:
                    continue
                G = src[trows[lo:hi]].astype(np.float64)
                q = src[qrows[lo:hi]].astype(np.float64)
                out[lo:hi] = self._dist(np.matmul(G, q[:, :, None])[..., 0])

        _parallel(work, list(range(0, len(qrows), step)))
        return out_m, out_e

    def row_dists(self, qrows):
        """d_model [len(qrows), nt] against every target."""
        q = self.H[np.asarray(qrows, np.int64)].astype(np.float64)
        out = np.empty((q.shape[0], self.nt), np.float64)
        step = max(1, CHUNK_BYTES // (8 * self.X.shape[1]))

        def work(lo):
            hi = min(lo + step, self.nt)
            out[:, lo:hi] = self._dist(q @ self.H[lo:hi].astype(np.float64).T)

        _parallel(work, list(range(0, self.nt, step)))
        return out


def decode(keys):
    """keys [.., kp] uint64 -> (d~ float64, global row int64, valid bool)."""
    keys = np.asarray(keys, np.uint64)
    valid = keys != KEY_INF
    dist = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    rows = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return dist, rows, valid


def check_lists(model, keys, qbits, qrows, check=None, complete=()):
    """The candidate lists keys [nq, kp] of the queries at T rows qrows [nq], against the model.

      shape        exactly min(kp, nt) valid keys, first; distinct rows inside [t_base, t_base + nt); d~ non-decreasing
                   (rows among equal d~ in any order: the ordered scan leaves ties so);
      accuracy     |d~ - d_model| <= tol for every listed key;
      premise      |d~ - d_exact| + 1e-6 <= prefilter_eps(qbits);
      completeness (the lists `complete`, full lists only) every non-member t has d_model(t) >= D - tol, D the list's
                   largest d~.
    `check`: the lists to check (default: every query that is not all-zero).  Raises AssertionError naming the first
    failures; returns the margins {"lists", "max_err_model", "max_err_exact", "tol", "eps", "completeness_min_gap"}."""
    keys = np.asarray(keys, np.uint64)
    nq, kp = keys.shape
    qrows = np.asarray(qrows, np.int64)
    if check is None:
        check = np.flatnonzero(~model.zero[qrows])
    check = np.asarray(check, np.int64)
    tol, eps = tolerance(model.d, qbits), prefilter_eps(qbits)
    dist, rows, valid = decode(keys[check])
    want = min(kp, model.nt)
    nvalid = valid.sum(1)
    bad = np.flatnonzero((nvalid != want) | ~valid[:, :want].all(1))
    assert bad.size == 0, "lists with %s valid keys, not %d (first at query %d)" % (
        np.unique(nvalid[bad]).tolist(), want, check[bad[0]])
    dist, rows = dist[:, :want], rows[:, :want]
    local = rows - model.t_base
    bad = np.flatnonzero(((local < 0) | (local >= model.nt)).any(1))
    assert bad.size == 0, "target row outside [t_base, t_base + nt) (query %d: %s)" % (check[bad[0]], rows[bad[0]])
    srt = np.sort(local, axis=1)
    bad = np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(1))
    assert bad.size == 0, "a row listed twice (query %d)" % check[bad[0]]
    bad = np.flatnonzero((dist[:, 1:] < dist[:, :-1]).any(1))
    assert bad.size == 0, "d~ decreases along the list of query %d" % check[bad[0]]
    dm, de = model.pair_dists(qrows[check], local)
    err_m, err_e = np.abs(dist - dm), np.abs(dist - de)
    bad = np.argwhere(err_m > tol)
    assert bad.size == 0, "%d keys off the model by more than tol = %.3g (query %d row %d: d~ %.9g, model %.9g)" % (
        len(bad), tol, check[bad[0][0]], rows[tuple(bad[0])], dist[tuple(bad[0])], dm[tuple(bad[0])])
    bad = np.argwhere(err_e + 1e-6 > eps)
    assert bad.size == 0, "%d keys break the certificate's premise eps = %.6g (query %d row %d: d~ %.9g, exact %.9g)" % (
        len(bad), eps, check[bad[0][0]], rows[tuple(bad[0])], dist[tuple(bad[0])], de[tuple(bad[0])])
    gap = np.inf
    complete = np.asarray(complete, np.int64)
    if complete.size and want == kp and model.nt > kp:
        cdist, crows, _ = decode(keys[complete])
        full = model.row_dists(qrows[complete])
        for i in range(complete.size):
            D = cdist[i, kp - 1]
            others = np.ones(model.nt, bool)
            others[crows[i] - model.t_base] = False
            lo = full[i][others].min()
            assert lo >= D - tol, "query %d missed target %d: d_model %.9g below the list's last d~ %.9g - tol" % (
                complete[i], model.t_base + np.flatnonzero(others)[np.argmin(full[i][others])], lo, D)
            gap = min(gap, lo - (D - tol))
    return {"lists": int(check.size), "max_err_model": float(err_m.max(initial=0)),
            "max_err_exact": float(err_e.max(initial=0)), "tol": tol, "eps": eps, "completeness_min_gap": float(gap)}


def check_ranges(model, qrows, theta, counts, rows, qbits):
    """Range-pass sets: query i (at T row qrows[i]) collected counts[i] targets with d~ <= theta[i], the first
    min(counts[i], RANGE_CAP) of them in rows[i] (global rows).  With A = {d_model <= theta - tol} and
    B = {d_model <= theta + tol + RANGE_SLACK}: A <= set <= B without duplicates when it fits, else |A| <= count <= |B|.
    Returns {"queries", "overflowed", "max_rows", "near_theta"} (near_theta: rows with d_model within 2e-4 below theta
    - tol over all queries, what a raised sfloor would lose)."""
    tol = tolerance(model.d, qbits)
    qrows = np.asarray(qrows, np.int64)
    full = model.row_dists(qrows)
    over, near, most = 0, 0, 0
    for i in range(len(qrows)):
        th, cnt = float(theta[i]), int(counts[i])
        A = np.flatnonzero(full[i] <= th - tol)
        B = full[i] <= th + tol + RANGE_SLACK
        near += int(((full[i] > th - tol - 2e-4) & (full[i] <= th - tol)).sum())
        most = max(most, cnt)
        if cnt > RANGE_CAP:
            over += 1
            assert A.size <= cnt <= int(B.sum()), "range query %d: count %d outside [|A| %d, |B| %d]" % (
                qrows[i], cnt, A.size, int(B.sum()))
            continue
        got = np.asarray(rows[i][:cnt], np.int64) - model.t_base
        assert np.all((got >= 0) & (got < model.nt)), "range query %d: row outside the targets" % qrows[i]
        assert np.unique(got).size == cnt, "range query %d: a row collected twice" % qrows[i]
        missing = np.setdiff1d(A, got)
        assert missing.size == 0, "range query %d (theta %.9g): missed %d rows of A, e.g. %d at d_model %.9g" % (
            qrows[i], th, missing.size, model.t_base + missing[0], full[i][missing[0]])
        extra = got[~B[got]]
        assert extra.size == 0, "range query %d (theta %.9g): collected row %d at d_model %.9g above theta + tol" % (
            qrows[i], th, model.t_base + extra[0], full[i][extra[0]])
    return {"queries": int(len(qrows)), "overflowed": over, "max_rows": most, "near_theta": near}
