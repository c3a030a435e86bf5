"""Embed, normalise and k-NN beyond d = 512 / k = 64 on dense rows (tests/_dense_rows.py), where a changed summation
order, a misplaced split-K hand-off or a wrong layout changes the distance bits.

Every k-NN case compares indices and distance bits with the oracle on sampled query rows (block edges, rows around
multiples of 32, 64 and 128, cluster members and duplicates, random rows), asserts from fdr_last_knn_trace which kernel
ran, and checks the result against float64 cosine distances (_assert_f64), which does not rely on the oracle."""
import numpy as np
import pytest

from fedrann_amd import _lib
from _dense_rows import mixed, sample_rows
from _guarded import knn_dev_guarded
from test_gpu_wide_knn import _assert_mfma_trace

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _d64(E, rows, T=None):
    """float64 cosine distances of rows `rows` of E to every row of T (default E), from the un-normalised rows, with
    the oracle's conventions: two zero rows 0, one zero row 1, clamped to [0, 1]."""
    X = E.astype(np.float64)
    Y = X if T is None else T.astype(np.float64)
    nx = np.sqrt(np.einsum("ij,ij->i", X[rows], X[rows]))
    ny = np.sqrt(np.einsum("ij,ij->i", Y, Y))
    G = X[rows] @ Y.T
    with np.errstate(divide="ignore", invalid="ignore"):
        D = 1.0 - G / (nx[:, None] * ny[None, :])
    zq, zt = nx == 0, ny == 0
    D[zq, :] = 1.0
    D[:, zt] = 1.0
    D[np.ix_(zq, zt)] = 0.0
    return np.clip(D, 0.0, 1.0)


def _assert_f64(E, rows, idx, dist, k, T=None, t_base=0):
    """The returned neighbours of the sampled query rows against float64 cosine distances d64.

    With u = 2^-24 and unit-norm rows, the canonical fp32 arithmetic is off the true distance by at most
    tau = (2d + 16) u:
      - the squared norm is an fma chain of d terms, relative error <= d u; 1 / sqrt of it, rounded to fp32, <= d u / 2
        + u + O(u^2); each normalised component x_k * rinv adds one rounding, u: every xhat is x / |x| times
        (1 + eta) with |eta| <= (d / 2 + 2) u, so xhat . yhat = cos (1 + eta_x)(1 + eta_y), off by <= (d + 4) u;
      - the fma chain of the dot product over d terms is off by <= d u sum |xhat_k yhat_k| <= d u (Cauchy-Schwarz on
        unit-norm rows, up to O(u^2));
      - 1 - c, with c within [-1, 1], and the clamp add at most u.
    In all <= (2d + 5) u + O(d^2 u^2) < tau.  So for every sampled row: every returned distance lies within tau of
    d64; every target with d64 < d64[k-th] - 2 tau is returned (d64[k-th]: the k-th smallest float64 distance of the
    row); and no returned target has d64 > d64[k-th] + 2 tau."""
    d = E.shape[1]
    tau = (2 * d + 16) * 2.0 ** -24
    D = _d64(E, rows, T)
    for i, r in enumerate(rows):
        got = idx[r].astype(np.int64) - t_base
        row = D[i]
        kth = np.partition(row, k - 1)[k - 1]
        assert np.all(np.abs(dist[r].astype(np.float64) - row[got]) <= tau), (r, np.abs(dist[r] - row[got]).max())
        must = np.flatnonzero(row < kth - 2 * tau)
        assert np.all(np.isin(must, got)), (r, np.setdiff1d(must, got)[:8])
        assert np.all(row[got] <= kth + 2 * tau), r


def _oracle_check(oracle, E, got, k, rows):
    Eh, _, zero = oracle.normalize(E)
    wi, wd = oracle.knn_normalized(Eh[rows], zero[rows], Eh, zero, k)
    gi, gd = got
    assert np.array_equal(gi[rows], wi), "indices differ in %d of %d cells" % (int((gi[rows] != wi).sum()), wi.size)
    assert np.array_equal(_bits(gd[rows]), _bits(wd)), "distance bits differ in %d cells" % int(
        (_bits(gd[rows]) != _bits(wd)).sum())


def _dense_case(n, d, k, seed):
    E, extra = mixed(n, d, seed, k)
    return E, sample_rows(n, seed, extra)


# ---- the wide route: the exact fp32 MFMA pass from 8192 targets ---------------------------------------------------
WIDE = [(9001, 128, 65), (8221, 128, 128), (9001, 256, 65), (8221, 256, 100), (9001, 256, 128), (8221, 500, 65),
        (9001, 500, 128)] + [(9001 if k % 2 else 8221, d, k) for d in (513, 640, 1000, 1023, 1024) for k in (20, 64, 65, 128)]


@pytest.mark.parametrize("n,d,k", WIDE)
def test_wide_dense_matches_oracle_and_float64(ctx, oracle, n, d, k):
    E, rows = _dense_case(n, d, k, 1000 * d + k)
    got = ctx.knn(E, k)
    _assert_mfma_trace(ctx, n, ctx.padded_dim(d), k)
    _oracle_check(oracle, E, got, k, rows)
    _assert_f64(E, rows, got[0], got[1], k)


def test_wide_merge_at_its_cap_eight_segments(ctx, oracle):
    """k = 128 with 8 target segments: nseg * k = 1024 = FDR_MERGE_WIDE_CAP keys staged per query by
    knn_merge_wide_kernel (a ragged block of 1000 queries against 9000 targets, the split-K kernel at d = 1000)."""
    import torch
    from fedrann_amd.distributed import HipEngine
    dev = torch.device("cuda", 0)
    n, d, k, nq = 9000, 1000, 128, 1000
    E, extra = mixed(n, d, 88, k)
    dp = ctx.padded_dim(d)
    Ehat = torch.zeros((n, dp), dtype=torch.float32, device=dev)
    zero = torch.zeros((n,), dtype=torch.uint8, device=dev)
    HipEngine(ctx, dev).normalize(torch.from_numpy(E).to(dev), Ehat, zero)
    q0 = 4000
    # (workspace and outputs hold 0xFF bytes between canaries, checked after the synchronise: tests/_guarded.py)
    idx, dst, _ = knn_dev_guarded(ctx, Ehat, zero, q0, nq, 0, d, k, stream=torch.cuda.current_stream(dev).cuda_stream)
    _assert_mfma_trace(ctx, nq, dp, k)
    tr = ctx.last_knn_trace()
    if ctx.device_info()["cus"] == 256:
        assert tr["exact_segments"] == 8, tr
    assert 1 <= tr["exact_segments"] and tr["exact_segments"] * k <= 1024, tr
    rows = q0 + sample_rows(nq, 5)
    Eh, _, oz = oracle.normalize(E)
    wi, wd = oracle.knn_normalized(Eh[rows], oz[rows], Eh, oz, k)
    gi, gd = idx.cpu().numpy(), dst.cpu().numpy()
    assert np.array_equal(gi[rows - q0], wi)
    assert np.array_equal(_bits(gd[rows - q0]), _bits(wd))
    full_i = np.zeros((n, k), np.int32)
    full_d = np.zeros((n, k), np.float32)
    full_i[q0:q0 + nq], full_d[q0:q0 + nq] = gi, gd
    _assert_f64(E, rows, full_i, full_d, k)


def test_wide_merge_single_segment(ctx, oracle):
    """One target segment (16169 rows at d = 1000, k = 128 on 256 CUs): the merge takes k keys from one list."""
    n, d, k = 16169, 1000, 128
    E, rows = _dense_case(n, d, k, 16169)
    got = ctx.knn(E, k)
    _assert_mfma_trace(ctx, n, ctx.padded_dim(d), k)
    tr = ctx.last_knn_trace()
    if ctx.device_info()["cus"] == 256:
        assert tr["exact_segments"] == 1, tr
    assert tr["exact_segments"] >= 1, tr
    _oracle_check(oracle, E, got, k, rows)
    _assert_f64(E, rows, got[0], got[1], k)


@pytest.mark.parametrize("d,k", [(1000, 100), (256, 128)])
def test_wide_dense_knn_dev_ragged_block(ctx, oracle, d, k):
    """fdr_knn_dev: a ragged query block (not a multiple of 32 rows) at t_base != 0, dense rows."""
    import torch
    from fedrann_amd.distributed import HipEngine
    dev = torch.device("cuda", 0)
    n, t_base = 9050, 777
    E, extra = mixed(n, d, d + k, k)
    dp = ctx.padded_dim(d)
    Ehat = torch.zeros((n, dp), dtype=torch.float32, device=dev)
    zero = torch.zeros((n,), dtype=torch.uint8, device=dev)
    HipEngine(ctx, dev).normalize(torch.from_numpy(E).to(dev), Ehat, zero)
    Eh, _, oz = oracle.normalize(E)
    for q0, q1 in ((0, 3001), (6033, 9050)):
        nq = q1 - q0
        # (workspace and outputs hold 0xFF bytes between canaries, checked after the synchronise: tests/_guarded.py)
        idx, dst, _ = knn_dev_guarded(ctx, Ehat, zero, q0, nq, t_base, d, k,
                                      stream=torch.cuda.current_stream(dev).cuda_stream)
        _assert_mfma_trace(ctx, nq, dp, k)
        rows = q0 + sample_rows(nq, q0, extra[(extra >= q0) & (extra < q1)] - q0)
        wi, wd = oracle.knn_normalized(Eh[rows], oz[rows], Eh, oz, k)
        gi, gd = idx.cpu().numpy(), dst.cpu().numpy()
        assert np.array_equal(gi[rows - q0], wi + t_base)
        assert np.array_equal(_bits(gd[rows - q0]), _bits(wd))
        full_i = np.zeros((n, k), np.int32)
        full_d = np.zeros((n, k), np.float32)
        full_i[q0:q1], full_d[q0:q1] = gi, gd
        _assert_f64(E, rows, full_i, full_d, k, t_base=t_base)


@pytest.mark.parametrize("d,k", [(256, 100), (1000, 65)])
def test_wide_dense_same_bits_in_every_mode(ctx, oracle, d, k):
    """exact, prefilter and auto, each with the duplicate-row layer off and forced: the same bits on dense rows."""
    n = 9001
    E, rows = _dense_case(n, d, k, 31 + d)
    results = []
    try:
        for mode in ("exact", "prefilter", "auto"):
            for dedup in ("off", "force"):
                ctx.set_knn_mode(mode)
                ctx.set_dedup_mode(dedup)
                results.append(ctx.knn(E, k))
                _assert_mfma_trace(ctx, n, ctx.padded_dim(d), k)
    finally:
        ctx.set_knn_mode("auto")
        ctx.set_dedup_mode("auto")
    for idx, dist in results[1:]:
        assert np.array_equal(idx, results[0][0])
        assert np.array_equal(_bits(dist), _bits(results[0][1]))
    _oracle_check(oracle, E, results[0], k, rows)
    _assert_f64(E, rows, results[0][0], results[0][1], k)


def test_wide_dense_subnormal_components(ctx, oracle):
    """Rows spanning more than 2^126 in magnitude (one component 2^27, the rest of a dense row scaled by 2^-100): their
    normalised components include fp32 subnormals.  Same bits as the oracle, and the float64 bound."""
    n, d, k = 9001, 1000, 65
    E, rows = _dense_case(n, d, k, 4242)
    rng = np.random.default_rng(4242)
    sub = rng.choice(n, size=96, replace=False)
    spikes = np.array([0, 511, 512, 999])
    E[sub] = E[rng.choice(n // 3, size=sub.size)] * np.float32(2.0 ** -100)
    E[sub, spikes[np.arange(sub.size) % spikes.size]] = np.float32(2.0 ** 27)
    Eh, _, _ = oracle.normalize(E)
    tiny = np.abs(Eh[sub])
    assert np.any((tiny > 0) & (tiny < np.finfo(np.float32).tiny))  # (the case this test is about)
    rows = np.unique(np.concatenate([rows, sub[:24]]))
    got = ctx.knn(E, k)
    _assert_mfma_trace(ctx, n, ctx.padded_dim(d), k)
    _oracle_check(oracle, E, got, k, rows)
    _assert_f64(E, rows, got[0], got[1], k)


# ---- the generic kernel below 8192 targets, and the fast route ---------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(3001, 1000, 100), (2999, 1500, 20), (2049, 2048, 128), (3001, 513, 65),
                                   (100, 1000, 100), (128, 2048, 128)])
def test_generic_dense_matches_oracle_and_float64(ctx, oracle, n, d, k):
    E, rows = _dense_case(n, d, k, n + d + k)
    got = ctx.knn(E, k)
    tr = ctx.last_knn_trace()
    assert tr["kind"] == "generic" and tr["generic"] == 1, tr
    assert np.all((ctx.last_query_paths(n) & 0x7F) == _lib.PATH_GENERIC)
    _oracle_check(oracle, E, got, k, rows)
    _assert_f64(E, rows, got[0], got[1], k)


def test_dense_route_threshold_at_8192_targets(ctx, oracle):
    """d = 1000, k = 100: 8191 targets on the generic kernel, 8192 on the split-K MFMA pass; both the oracle's bits."""
    d, k = 1000, 100
    E, extra = mixed(8192, d, 8191, k)
    for n, kind in ((8191, "generic"), (8192, "exact")):
        got = ctx.knn(E[:n], k)
        tr = ctx.last_knn_trace()
        assert tr["kind"] == kind and tr["generic"] == (kind == "generic"), tr
        rows = sample_rows(n, n, extra[extra < n])
        _oracle_check(oracle, E[:n], got, k, rows)
        _assert_f64(E[:n], rows, got[0], got[1], k)


@pytest.mark.parametrize("n,d,k", [(9001, 128, 20), (9001, 500, 50)])
def test_fast_route_dense_float64(ctx, oracle, n, d, k):
    """k <= 64 at d <= 512 (the fast passes) on the same dense rows: the oracle's bits and the float64 bound."""
    E, rows = _dense_case(n, d, k, 7 * d + k)
    got = ctx.knn(E, k)
    assert ctx.last_knn_trace()["generic"] == 0
    _oracle_check(oracle, E, got, k, rows)
    _assert_f64(E, rows, got[0], got[1], k)


# ---- normalize_rows_kernel ---------------------------------------------------------------------------------------
def _unpermute(Eh_dev, dp):
    """Ehat[r, 8g + 4h + s] = xhat[r, 8g + 2s + h]: back to component order."""
    p = np.arange(dp)
    src = 8 * (p >> 3) + 2 * (p & 3) + ((p >> 2) & 1)
    out = np.empty_like(Eh_dev)
    out[:, src] = Eh_dev
    return out


@pytest.mark.parametrize("d", [1, 7, 100, 128, 129, 255, 500, 512, 513, 1000, 1023, 1024, 1025, 2047, 2048])
def test_normalize_dev_layout_padding_and_zero_flags(ctx, oracle, d):
    """fdr_normalize_dev against oracle.normalize: bit-equal components after undoing the layout permutation, exact +0
    in components d .. DP-1, the oracle's zero flags -- on a row count that is no multiple of the row block, with 16-byte
    aligned buffers (the vector form when d % 4 == 0) and with buffers offset by one float (the scalar form).  Rows:
    dense rows of mixed magnitudes, all-zero rows, rows whose squared norm underflows to 0 (flagged zero on both
    sides), rows whose squared norm is a sum of fp32 subnormals, and rows with normalised subnormal components."""
    import torch
    dev = torch.device("cuda", 0)
    dp = ctx.padded_dim(d)
    rng = np.random.default_rng(d)
    n = 203  # (no multiple of RB = 64, 32, 16, 8 or 4)
    E = (rng.standard_normal((n, d)) * np.exp2(rng.uniform(-8, 8, size=(n, d)))).astype(np.float32)
    E[3] = 0.0
    E[n - 1] = 0.0
    E[10] = np.float32(2.0 ** -80)    # x * x = 2^-160: the squared norm underflows to 0
    E[11] = np.float32(-2.0 ** -70)   # x * x = 2^-140: subnormal squares
    E[12] = np.float32(2.0 ** -100)
    E[12, d // 2] = np.float32(2.0 ** 30)  # normalised: 1 and subnormals (when d > 1)
    E[13] = E[12] * np.float32(-1.0)
    want, _, wzero = oracle.normalize(E)
    for off in (0, 1):
        Ebuf = torch.zeros(n * d + 4, dtype=torch.float32, device=dev)
        Ebuf[off:off + n * d] = torch.from_numpy(E.reshape(-1)).to(dev)
        Hbuf = torch.full((n * dp + 4,), float("nan"), dtype=torch.float32, device=dev)
        zero = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        ctx.normalize_dev(Ebuf.data_ptr() + 4 * off, n, d, Hbuf.data_ptr() + 4 * off, zero.data_ptr(),
                          torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        H = Hbuf[off:off + n * dp].cpu().numpy().reshape(n, dp)
        X = _unpermute(H, dp)
        assert np.array_equal(_bits(X[:, :d]), _bits(want)), (off, np.argwhere(_bits(X[:, :d]) != _bits(want))[:8])
        assert np.all(_bits(X[:, d:]) == 0), off  # (+0, not -0 and not NaN)
        assert np.array_equal(zero.cpu().numpy(), wzero), off
        assert wzero[3] == 1 and wzero[10] == 1 and wzero[12] == 0
        assert np.isnan(Hbuf[:off].cpu().numpy()).all() and np.isnan(Hbuf[off + n * dp:].cpu().numpy()).all()


# ---- embed_csr_wide_kernel at DP = 1024 and 2048 -----------------------------------------------------------------
def _embed_inputs(d, seed, n_extra=41, long_rows=(0, 1, 255, 256, 257, 1023, 1024, 1025, 5000)):
    """A projection from the reference's recipe (oracle.precompute_matrix: ~d / sqrt(F) entries per feature row, its
    columns over all accumulator slots) and rows of the given lengths plus random ones, an odd row count."""
    rng = np.random.default_rng(seed)
    L = 4000
    counts = rng.integers(2, 61, size=L)
    from oracle import oracle as O
    P = O.precompute_matrix(counts, d)
    F = 2 * L
    lens = list(long_rows) + list(rng.integers(0, 400, size=n_extra))
    if len(lens) % 2 == 0:
        lens.append(3)
    rows = [np.sort(rng.choice(F, size=int(min(n, F)), replace=False)) for n in lens]
    return P, F, rows


def _assert_embed_f64(E, indptr, indices, P, F, d):
    """|E - (A . P in float64)| <= m 2^-24 sum |terms| per entry, m the entry's number of terms."""
    import scipy.sparse as sp
    n = indptr.size - 1
    A = sp.csr_matrix((np.ones(indices.size), indices, indptr), shape=(n, F))
    Pm = sp.csr_matrix((P[2].astype(np.float64), P[1], P[0]), shape=(F, d))
    exact = (A @ Pm).toarray()
    mag = (A @ abs(Pm)).toarray()
    m = (A @ (Pm != 0).astype(np.float64)).toarray()
    assert np.all(np.abs(E.astype(np.float64) - exact) <= m * 2.0 ** -24 * mag)


@pytest.mark.parametrize("d", [513, 640, 1000, 1024, 1025, 1500, 2048])
def test_embed_wide_matches_oracle_raw_and_compacted(ctx, oracle, d):
    P, F, rows = _embed_inputs(d, d)
    indptr, indices = oracle.rows_to_csr(rows)
    ctx.projection_load(P[0], P[1], P[2], F, d)
    want = oracle.embed(indptr, indices, P, F, d)
    assert np.any(np.diff(P[0]) > 1) and P[1].max() >= min(d, 1024) - 64  # (multi-entry rows reaching high slots)
    E = ctx.embed(indptr, indices.astype(np.int32))
    assert np.array_equal(_bits(E), _bits(want)), np.argwhere(_bits(E) != _bits(want))[:8]
    cip, cix = ctx.csr_compact(indptr, indices.astype(np.int32))
    assert np.array_equal(_bits(ctx.embed(cip, cix)), _bits(want))
    assert not E[0].any()
    _assert_embed_f64(E, indptr, indices, P, F, d)


def test_embed_wide_pipelined_upload(ctx, oracle):
    """d = 1000 above the 1 M-id threshold of fdr_embed's pipelined host upload."""
    d = 1000
    rng = np.random.default_rng(1000)
    P, F, _ = _embed_inputs(d, 77, n_extra=0, long_rows=())
    lens = rng.integers(0, 300, size=8001)
    lens[5] = 0
    lens[4000] = F
    rows = [np.sort(rng.choice(F, size=int(n), replace=False)) for n in lens]
    indptr, indices = oracle.rows_to_csr(rows)
    assert indices.size > (1 << 20)
    ctx.projection_load(P[0], P[1], P[2], F, d)
    E = ctx.embed(indptr, indices.astype(np.int32))
    want = oracle.embed(indptr, indices, P, F, d)
    assert np.array_equal(_bits(E), _bits(want))


@pytest.mark.parametrize("d", [1000, 2048])
def test_embed_wide_matches_reference_golden(ctx, oracle, d):
    """tests/golden/embed_wide.npz: E of the reference's get_feature_matrix at d = 1000 and 2048."""
    from test_oracle import assert_wide_golden, wide_golden_case
    indptr, indices, P, F = wide_golden_case(oracle, d)
    ctx.projection_load(P[0], P[1], P[2], F, d)
    assert_wide_golden(ctx.embed(indptr, indices.astype(np.int32)), d)
