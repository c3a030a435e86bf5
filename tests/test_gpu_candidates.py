"""The prefilter mode's intermediate results against the float64 model of tests/_candidate_model.py.

The end-to-end tests (test_gpu_paths.py, test_gpu_parity.py) see a fault of the fp16 candidate pass or the range pass
only when it changes a final answer; here the context captures (fdr_set_knn_capture) the merged candidate lists and
the range sets of every call, and each is checked directly: the lists' shape, every listed d~ within tol of the model,
the certificate's premise |d~ - d_exact| + 1e-6 <= eps, completeness against all targets, and the range sets bracketed
by {d_model <= theta -+ tol}.  On every candidate-pass kernel variant (CASES), the adversarial rounding sets, and the
list / size edges; the duplicate-row layer is off throughout (the capture then describes the call's own rows)."""
import zlib

import numpy as np
import pytest

import _candidate_model as M
from _guarded import knn_dev_guarded
from _paths_rows import CASES, MIX, RESERVED, _normalize, _paths_input
from _strata import stratified_rows
from fedrann_amd import _lib
from test_gpu_parity import _adversarial_rows

pytestmark = pytest.mark.gpu

CAPTURE = _lib.CAPTURE_CANDIDATES | _lib.CAPTURE_RANGE


def _run(ctx, Ehat, zero, q0, nq, d, k, t_base, mode="prefilter", capture=CAPTURE):
    """fdr_knn_dev of rows [q0, q0 + nq) against all rows, dedup off, capture as asked; the workspace is freed before
    the capture is read.  (idx, dist, paths, trace, keys, qbits, ranges) on the host."""
    import torch
    ctx.set_knn_mode(mode)
    ctx.set_dedup_mode("off")
    ctx.set_knn_capture(capture)
    try:
        # (workspace and outputs hold 0xFF bytes between canaries, checked after the synchronise: tests/_guarded.py)
        idx, dst, ws = knn_dev_guarded(ctx, Ehat, zero, q0, nq, t_base, d, k)
        paths = ctx.last_query_paths(nq)
        del ws
        torch.cuda.empty_cache()
        tr = ctx.last_knn_trace()
        keys = qbits = ranges = None
        if capture:
            keys, qbits = ctx.last_candidates(nq, tr["kp"])
            if tr["range_queries"] > 0:
                ranges = ctx.last_range_sets(tr["range_queries"])
    finally:
        ctx.set_knn_capture(0)
        ctx.set_dedup_mode("auto")
        ctx.set_knn_mode("auto")
    return idx.cpu().numpy(), dst.cpu().numpy(), paths, tr, keys, qbits, ranges


def _check(ctx, Ehat, zero, q0, nq, d, k, t_base, tag, complete=None, n_complete=256, n_range=128, seed=0):
    """One capturing call and every check of it; `complete`: the lists to test for completeness (None: per path
    stratum, at least n_complete of them, plus the block's first and last rows).  Returns (report, trace)."""
    _, _, paths, tr, keys, qbits, ranges = _run(ctx, Ehat, zero, q0, nq, d, k, t_base)
    assert tr["kind"] == "prefilter", (tag, tr)
    model = M.Model(Ehat.cpu().numpy(), zero.cpu().numpy(), d, t_base=t_base)
    qrows = q0 + np.arange(nq)
    if complete is None:
        rng = np.random.default_rng(seed)
        picked, _, _ = stratified_rows(paths, per=64, seed=seed + 1)
        more = rng.choice(nq, size=min(nq, n_complete), replace=False)
        complete = np.unique(np.concatenate([picked, more, [0, nq - 1]]))
    complete = np.asarray(complete, np.int64)
    complete = complete[~model.zero[qrows[complete]]]
    assert complete.size >= min(n_complete, int((~model.zero[qrows]).sum())), (tag, complete.size)
    rep = M.check_lists(model, keys, qbits, qrows, complete=complete)
    rep["complete"] = int(complete.size)
    rep["qbits"] = qbits
    if ranges is not None:
        rq, th, cnt, rows = ranges
        if tr["exact_fallback"] != "whole":  # (the whole-call fallback recodes every row FDR_PATH_EXACT)
            code = paths & 0x7F
            assert np.array_equal(np.sort(rq), np.flatnonzero((code == _lib.PATH_RANGE) |
                                                              (code == _lib.PATH_RANGE_OVERFLOW))), tag
        rng = np.random.default_rng(seed + 2)
        over = np.flatnonzero(cnt > M.RANGE_CAP)[:64]
        some = rng.choice(rq.size, size=min(rq.size, n_range), replace=False)
        sel = np.unique(np.concatenate([over, some]))
        rep["range"] = M.check_ranges(model, q0 + rq[sel].astype(np.int64), th[sel], cnt[sel], rows[sel], qbits)
        assert rep["range"]["overflowed"] >= min(64, int((cnt > M.RANGE_CAP).sum())), (tag, rep["range"])
    print("%s: margins |d~ - d_model| <= %.3g (tol %.3g), |d~ - d_exact| <= %.3g (eps %.6g); %s" % (
        tag, rep["max_err_model"], rep["tol"], rep["max_err_exact"], rep["eps"],
        {key: rep[key] for key in ("lists", "complete", "qbits", "completeness_min_gap", "range") if key in rep}))
    return rep, tr


def _variant(trace):
    return {key: trace[key] for key in ("dp", "pass_waves", "pass_wps", "pass_units", "pass_list_keys", "pass_pingpong")}


def _rank_form(E, d, seed=7):
    """E's rows as a query block between 2 x 2048 further target rows (test_gpu_paths.py's rank form)."""
    import torch
    g = torch.Generator(device=E.device)
    g.manual_seed(seed)
    pad = torch.zeros((4096, d), dtype=torch.float32, device=E.device)
    pad[:, :d - RESERVED] = torch.randn((4096, 24), device=E.device, generator=g) @ \
        torch.randn((24, d - RESERVED), device=E.device, generator=g)
    return torch.cat([pad[:2048], E, pad[2048:]]).contiguous()


@pytest.mark.parametrize("name,d,k,scale,mix,shape,one_launch,fallback", CASES, ids=[c[0] for c in CASES])
def test_candidates_per_variant(ctx, name, d, k, scale, mix, shape, one_launch, fallback):
    """Every candidate-pass kernel variant at the size the planner picks it, all-pairs and rank form."""
    cus = ctx.device_info()["cus"]
    n = int(scale * 512 * cus)
    if mix == "whole":
        plateau, overflow = (0, 0), -(-(n // 2 + 2048) // 1100)
    else:
        plateau, overflow = MIX[mix]
    want = dict(zip(("pass_waves", "pass_wps", "pass_units", "pass_list_keys", "pass_pingpong"), shape),
                dp=ctx.padded_dim(d))
    E = _paths_input(n, d, seed=zlib.crc32(name.encode()) % 1000, plateau=plateau, overflow=overflow)
    Ehat, zero = _normalize(ctx, E)
    _, tr = _check(ctx, Ehat, zero, 0, n, d, k, 0, name + "/all-pairs")
    assert _variant(tr) == want, (name, _variant(tr), want)
    assert tr["range_queries"] > 0, tr
    T = _rank_form(E, d)
    del E, Ehat, zero
    That, tzero = _normalize(ctx, T)
    _, tr = _check(ctx, That, tzero, 2048, n, d, k, 1 << 20, name + "/rank", seed=1)
    assert _variant(tr) == want, (name, _variant(tr), want)


ADVERSARIAL = [(kind, d) for kind in ("fp16_midpoints", "fp16_subnormals", "dense") for d in (128, 256, 500)]


@pytest.mark.parametrize("kind,d", ADVERSARIAL, ids=["%s-%d" % a for a in ADVERSARIAL])
def test_candidates_on_adversarial_rows(ctx, kind, d):
    """The rounding-sensitive sets of test_gpu_parity.py on the device (the certificate's eps, knn_plan.inc): every
    list of 3000 rows complete, k = 20 and 50; at d = 256 / 500 also at the ping-pong kernel's size."""
    import torch
    rng = np.random.default_rng(d + 7 * len(kind))
    E = torch.from_numpy(_adversarial_rows(kind, 3000, d, rng)).to("cuda")
    Ehat, zero = _normalize(ctx, E)
    for k in (20, 50):
        _check(ctx, Ehat, zero, 0, 3000, d, k, 0, "%s-%d/k%d" % (kind, d, k), complete=np.arange(3000))
    if d >= 256:
        n = int(1.15 * 512 * ctx.device_info()["cus"])
        E = torch.from_numpy(_adversarial_rows(kind, n, d, rng)).to("cuda")
        Ehat, zero = _normalize(ctx, E)
        _, tr = _check(ctx, Ehat, zero, 0, n, d, 20, 0, "%s-%d/pingpong" % (kind, d), seed=3)
        assert tr["pass_pingpong"] == 1, tr


def _dense(n, d, seed):
    import torch
    rng = np.random.default_rng(seed)
    return torch.from_numpy(_adversarial_rows("dense", n, d, rng)).to("cuda")


def _kp(k):
    return (k + (12 if k + 12 <= (32 if k + 8 <= 32 else 64) else 8) + 1) & ~1


EDGE_K = (1, 20, 21, 24, 25, 52, 56)


@pytest.mark.parametrize("k", EDGE_K)
def test_candidates_list_and_size_edges(ctx, k):
    """16- and 32-key lists with dead entries and full (K' = 14 ... 64); targets nt = K', 33, 97 and 20 013 rows (not
    a multiple of 32, several target segments); rank-form query blocks of 1 and 33 rows; every check on every query."""
    kp = _kp(k)
    assert kp == {1: 14, 20: 32, 21: 30, 24: 32, 25: 38, 52: 64, 56: 64}[k]
    d = 100
    for nt in sorted({kp, 33, 97}):
        if nt < kp:  # (the prefilter mode needs nt >= K')
            continue
        Ehat, zero = _normalize(ctx, _dense(nt, d, seed=nt + k))
        _, tr = _check(ctx, Ehat, zero, 0, nt, d, k, 0, "k%d/nt%d" % (k, nt), complete=np.arange(nt))
        assert tr["kp"] == kp, tr
    n = 20013
    Ehat, zero = _normalize(ctx, _dense(n, d, seed=k))
    _, tr = _check(ctx, Ehat, zero, 0, n, d, k, 0, "k%d/n%d" % (k, n), complete=np.arange(0, n, 7))
    assert tr["pass_segments"] > 1, tr
    for q0, nq in ((0, 1), (n - 1, 1), (5000, 33), (n - 33, 33)):
        _check(ctx, Ehat, zero, q0, nq, d, k, 1 << 20, "k%d/block%d+%d" % (k, q0, nq), complete=np.arange(nq))


def _graded_plateaus(d, clusters, members, graded, seed):
    """`clusters` centres q = 3 e_u + 2 e_v, each with `members` rows q +- e_j (an exact distance plateau) and `graded`
    rows q +- a e_j, a from 1 to 1.1: distances from q spread densely over 7e-3 above the plateau, so that each centre's
    range set {d~ <= d~(K) + M} has rows close under its theta (what the range kernels' sfloor decides)."""
    rng = np.random.default_rng(seed)
    free = d - RESERVED
    rows, seen = [], set()
    while len(seen) < clusters:
        u, v = (int(x) for x in rng.choice(free, 2, replace=False))
        if (u, v) in seen:
            continue
        seen.add((u, v))
        q = np.zeros(d, np.float32)
        q[u], q[v] = 3, 2
        rows.append(q)
        opts = np.array([(j, s) for j in range(free) if j not in (u, v) for s in (-1, 1)])
        pick = opts[rng.choice(len(opts), members + graded, replace=False)]
        alpha = np.concatenate([np.ones(members), 1 + 0.1 * np.arange(1, graded + 1) / graded])
        for (j, s), a in zip(pick, alpha):
            t = q.copy()
            t[j] = s * a
            rows.append(t)
    return np.stack(rows)


@pytest.mark.parametrize("d,clusters", [(128, 12), (256, 48)])
def test_range_sets_close_under_theta(ctx, d, clusters):
    """Range queries whose sets have rows just under theta (within 2e-4): a range kernel that drops them (a raised
    sfloor) misses rows of A.  48 clusters: enough range queries for the ping-pong range kernel."""
    import torch
    P = _graded_plateaus(d, clusters, 100, 140, seed=d)
    rng = np.random.default_rng(d + 1)
    bg = np.zeros((4000, d), np.float32)
    bg[:, :d - RESERVED] = rng.standard_normal((4000, d - RESERVED))
    E = np.concatenate([P, bg])
    E = torch.from_numpy(E[rng.permutation(E.shape[0])]).to("cuda")
    Ehat, zero = _normalize(ctx, E)
    n = E.shape[0]
    rep, tr = _check(ctx, Ehat, zero, 0, n, d, 20, 0, "graded-%d" % d, n_range=4096)
    assert tr["range_queries"] >= clusters and rep["range"]["near_theta"] > 0, (tr, rep["range"])
    if clusters >= 48:
        print("graded-%d: range chunks %d, ping-pong %d" % (d, tr["range_chunks"], tr["range_pp_chunks"]))


@pytest.mark.parametrize("d", [100, 256, 500])
def test_capture_changes_nothing_and_outlives_the_workspace(ctx, d):
    """Per padded dimension: indices, distance bits, path codes and trace identical with capture on and off; the
    capture read after the workspace is gone (_run frees it first) and again after a later exact call is refused."""
    cus = ctx.device_info()["cus"]
    n = int(0.3 * 512 * cus)
    E = _paths_input(n, d, seed=d, plateau=(12, 150), overflow=1)  # (d = 100: 2 x 94 members at most)
    Ehat, zero = _normalize(ctx, E)
    off = _run(ctx, Ehat, zero, 0, n, d, 20, 0, capture=0)
    on = _run(ctx, Ehat, zero, 0, n, d, 20, 0)
    assert np.array_equal(off[0], on[0])
    assert np.array_equal(off[1].view(np.uint32), on[1].view(np.uint32))
    assert np.array_equal(off[2], on[2]) and off[3] == on[3]
    assert on[3]["range_queries"] > 0 and on[6] is not None
    # the capture of a non-capturing call, of an exact-mode call and of a failed call: FDR_E_STATE
    with pytest.raises(_lib.FedrannHipError, match="captured no"):
        _run(ctx, Ehat, zero, 0, n, d, 20, 0, capture=0)
        ctx.last_candidates(n, on[3]["kp"])
    ctx.set_knn_capture(CAPTURE)
    try:
        ctx.set_knn_mode("exact")
        ctx.knn(np.random.default_rng(1).standard_normal((3000, d)).astype(np.float32), 10)
        with pytest.raises(_lib.FedrannHipError, match="captured no"):
            ctx.last_candidates(3000, 22)
        with pytest.raises(_lib.FedrannHipError, match="captured no"):
            ctx.last_range_sets(1)
        ctx.set_knn_mode("prefilter")
        rows = np.random.default_rng(2).standard_normal((3000, d)).astype(np.float32)
        ctx.knn(rows, 10)
        tr = ctx.last_knn_trace()
        assert ctx.last_candidates(3000, tr["kp"])[0].shape == (3000, tr["kp"])
        with pytest.raises(_lib.FedrannHipError):
            ctx.knn(rows, 0)
        with pytest.raises(_lib.FedrannHipError, match="captured no"):
            ctx.last_candidates(3000, tr["kp"])
    finally:
        ctx.set_knn_capture(0)
        ctx.set_knn_mode("auto")
