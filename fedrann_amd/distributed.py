"""Row-sharded embed + k-NN over the GPUs of one node (one process per GPU).

The path shards by read rows: rank g embeds and normalises rows [g*S, (g+1)*S) of the feature
matrix, the normalised embeddings (and their zero-row flags) are exchanged with ONE all-gather
(RCCL over xGMI when the process group's backend is "nccl"), and each rank then searches its own
rows against all N targets.  No merge step: a query's full top-k is produced on its owner rank.  When the
gathered rows repeat (>= 5 % duplicates; the sparse projections of overlapping reads often coincide), the
ranks split the UNIQUE rows instead and exchange those results with a second, small all-gather (see step()).

torch is used for device memory, streams and torch.distributed only; the arithmetic is in
libfedrann_hip.so (HipEngine).  The engine is injected so that the sharding / exchange logic can be
exercised on CPU with the gloo backend (tests/test_distributed.py drives it with an oracle-backed
engine); HipEngine itself refuses to run without a GPU.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import _lib


def shard_rows(n_rows, world_size, align=32):
    """Contiguous row blocks, equal size S (a multiple of `align`, so fwd/rev row pairs and the
    32-row tiles never straddle ranks); trailing ranks may hold fewer (or no) real rows."""
    S = -(-n_rows // world_size)
    S = -(-S // align) * align
    return S, [(min(n_rows, g * S), min(n_rows, (g + 1) * S)) for g in range(world_size)]


class HipEngine:
    """The three device stages on one GPU, on torch-owned HBM buffers and torch's current stream."""

    def __init__(self, context, device):
        if not torch.cuda.is_available():
            raise _lib.FedrannHipError("HipEngine needs a GPU: there is no CPU fallback")
        self.ctx = context
        self.device = torch.device(device)
        self._ws = None

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def padded_dim(self, d):
        return self.ctx.padded_dim(d)

    def embed(self, indptr, indices, n_rows, d):
        E = torch.empty((n_rows, d), dtype=torch.float32, device=self.device)
        if n_rows:
            self.ctx.embed_dev(n_rows, indptr.data_ptr(), indices.data_ptr(), E.data_ptr(), self._stream())
        return E

    def normalize(self, E, Ehat_out, zero_out):
        n, d = E.shape
        if n:
            self.ctx.normalize_dev(E.data_ptr(), n, d, Ehat_out.data_ptr(), zero_out.data_ptr(),
                                   self._stream())

    def knn(self, Qhat, qzero, nq, That, tzero, nt, d, k):
        idx = torch.empty((nq, k), dtype=torch.int32, device=self.device)
        dst = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        if nq == 0:
            return idx, dst
        need = self.ctx.knn_workspace_bytes(nq, nt, d, k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.ctx.knn_dev(Qhat.data_ptr(), qzero.data_ptr(), nq, That.data_ptr(), tzero.data_ptr(), nt,
                         0, d, k, idx.data_ptr(), dst.data_ptr(), self._ws.data_ptr(),
                         self._ws.numel(), self._stream())
        return idx, dst

    # -- duplicate-row classes across ranks (fdr_knn_classes_dev / _unique_dev / _expand_dev) --------------
    def knn_classes(self, That, tzero, nt, d, k, nq_max):
        """Build the classes of the gathered target set; returns the number of unique rows, 0 = use knn()."""
        need = self.ctx.knn_workspace_bytes(nq_max, nt, d, k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.ctx.knn_classes_dev(That.data_ptr(), tzero.data_ptr(), nt, d, k, nq_max, self._ws.data_ptr(),
                                        self._ws.numel(), self._stream())

    def knn_unique(self, u_lo, u_hi, k, out_idx, out_dst):
        """k-NN of the unique rows [u_lo, u_hi) into the first u_hi - u_lo rows of out_idx / out_dst."""
        if u_hi > u_lo:
            self.ctx.knn_unique_dev(u_lo, u_hi, out_idx.data_ptr(), out_dst.data_ptr(), self._stream())

    def knn_expand(self, q0, nq, k, packed_u_all):
        """packed_u_all int32 [n_unique (padded), 2 k]: a unique row's k indices, then its k distance bit patterns."""
        idx = torch.empty((nq, k), dtype=torch.int32, device=self.device)
        dst = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        if nq:
            base = packed_u_all.data_ptr()
            self.ctx.knn_expand_dev(q0, nq, 0, base, base + 4 * k, idx.data_ptr(), dst.data_ptr(), self._stream(),
                                    u_row_stride=2 * k)
        return idx, dst


class ShardedPipeline:
    """embed -> normalise -> all-gather -> k-NN for this rank's row block."""

    def __init__(self, engine, n_rows_total, d, k, rank=0, world_size=1, group=None, device="cpu"):
        self.engine, self.n, self.d, self.k = engine, int(n_rows_total), int(d), int(k)
        self.rank, self.world, self.group = rank, world_size, group
        self.device = torch.device(device)
        self.S, self.blocks = shard_rows(self.n, world_size)
        self.lo, self.hi = self.blocks[rank]
        self.dp = engine.padded_dim(d)
        G, S = world_size, self.S
        # gathered buffers (all ranks' normalised rows, row i of the matrix at position i)
        self.Ehat_all = torch.zeros((G * S, self.dp), dtype=torch.float32, device=self.device)
        self.zero_all = torch.zeros((G * S,), dtype=torch.uint8, device=self.device)
        if G > 1:
            self.Ehat_loc = torch.zeros((S, self.dp), dtype=torch.float32, device=self.device)
            self.zero_loc = torch.zeros((S,), dtype=torch.uint8, device=self.device)
        else:
            self.Ehat_loc, self.zero_loc = self.Ehat_all, self.zero_all
        self._pu = self._pu_loc = self._iu_loc = self._du_loc = None  # unique-row results (sized on first use)

    def step(self, indptr_local, indices_local):
        """indptr_local / indices_local: this rank's CSR rows (indptr rebased to 0) as tensors on
        the pipeline's device.  Returns (idx int32 [rows, k], dist float32 [rows, k], E)."""
        nloc = self.hi - self.lo
        E = self.engine.embed(indptr_local, indices_local, nloc, self.d)
        self.engine.normalize(E, self.Ehat_loc, self.zero_loc)
        if self.world > 1:
            # two collectives: the rows (S x DP fp32 per rank; the class layer compares whole rows, so the search
            # cannot start on less) and the zero flags (S bytes; packing them behind a rank's rows would leave the
            # gathered rows non-contiguous, and the kernels address row i at i * DP)
            w = dist.all_gather_into_tensor(self.zero_all, self.zero_loc, group=self.group, async_op=True)
            dist.all_gather_into_tensor(self.Ehat_all, self.Ehat_loc, group=self.group)
            w.wait()
        q0 = self.rank * self.S
        if self.world > 1 and hasattr(self.engine, "knn_classes"):
            # Split the UNIQUE rows over the ranks instead of searching every duplicate query row on every
            # rank that holds a member of its class: all ranks build the same class tables from the gathered
            # rows (the decision to do so is a function of the exact unique count: the same on every rank), each
            # searches its share of the unique rows, ONE more all-gather exchanges the shares (a unique row's k
            # indices and k distance bit patterns side by side), and each rank expands its own rows.
            nq_max = -(-self.n // self.world)
            nu = self.engine.knn_classes(self.Ehat_all, self.zero_all, self.n, self.d, self.k, nq_max)
            if nu > 0:
                Su, k = -(-nu // self.world), self.k
                u_lo, u_hi = min(nu, self.rank * Su), min(nu, (self.rank + 1) * Su)
                if self._pu is None or self._pu.shape[0] != Su * self.world:
                    self._pu = torch.zeros((Su * self.world, 2 * k), dtype=torch.int32, device=self.device)
                    self._pu_loc = torch.zeros((Su, 2 * k), dtype=torch.int32, device=self.device)
                    self._iu_loc = torch.zeros((Su, k), dtype=torch.int32, device=self.device)
                    self._du_loc = torch.zeros((Su, k), dtype=torch.float32, device=self.device)
                self.engine.knn_unique(u_lo, u_hi, k, self._iu_loc, self._du_loc)
                self._pu_loc[:, :k] = self._iu_loc
                self._pu_loc[:, k:] = self._du_loc.view(torch.int32)
                dist.all_gather_into_tensor(self._pu, self._pu_loc, group=self.group)
                idx, dst = self.engine.knn_expand(q0, nloc, k, self._pu)  # (unique row u sits at row u)
                return idx, dst, E
        idx, dst = self.engine.knn(self.Ehat_all[q0:q0 + nloc], self.zero_all[q0:q0 + nloc], nloc,
                                   self.Ehat_all, self.zero_all, self.n, self.d, self.k)
        return idx, dst, E


def sparse_rank_blocks(n_rows, rank, world, block_rows=None):
    """(lo, hi, blocks): the rows [lo, hi) of `rank` in shard_rows(n_rows, world), and the query blocks
    sparse_knn_rank searches them in: consecutive ranges of at most block_rows rows (None: one block).  The blocks
    of all ranks tile [0, n_rows).  Needs no GPU."""
    rank, world = int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("need 0 <= rank < world, got rank %d of %d" % (rank, world))
    if block_rows is not None and int(block_rows) < 1:
        raise ValueError("block_rows must be at least 1")
    lo, hi = shard_rows(int(n_rows), world)[1][rank]
    step = max(hi - lo, 1) if block_rows is None else int(block_rows)
    return lo, hi, [(a, min(hi, a + step)) for a in range(lo, hi, step)]


def sparse_knn_rank(ctx, indptr, indices, values, n_features, k, rank, world, metric="cosine", block_rows=None):
    """This rank's share of Context.knn_sparse on the whole CSR: (lo, hi, idx int32 [hi - lo, k], dist float32
    [hi - lo, k]) for the rows [lo, hi) of `rank` in shard_rows(n, world), the dense pipeline's split; neighbour
    indices are global rows.  The rank builds the index of the WHOLE CSR (Context.sparse_index) and searches its own
    rows in query blocks of at most block_rows rows (None: one block), which bounds the device's result buffers.

    No collective and no process group: a search is one independent wave per query, so the ranks' results,
    concatenated in rank order, are the one-GPU answer bit for bit.  The price is a replicated index: EVERY rank
    uploads the full CSR and holds about 52 (cosine, weighted Jaccard) or 44 (Jaccard) device bytes per stored entry,
    plus the sort's temporary storage of about 12 more (64 measured at 1 M reads, cosine), and pays the O(nnz) build; only
    the search, sum over the features of df^2, is divided by the ranks (by row count, not by cost).  The index is
    freed before the call returns.

    The alternative is sparse_knn_target_shard, which divides the TARGETS: a rank indexes only its own rows, so it
    holds 1 / world of the index and pays 1 / world of the build, but it sees every query (all n rows go through
    SparseIndex.query, their upload included), and the ranks exchange k candidates per query and rank, which
    merge_sparse_topk merges exactly.  Replicated index: the work is divided by queries and nothing is exchanged;
    sharded index: memory and build are divided, the read set is no longer bounded by one GPU's memory."""
    with ctx.sparse_index(indptr, indices, values, n_features, metric=metric) as index:  # (checks the CSR first)
        lo, hi, blocks = sparse_rank_blocks(index.n, rank, world, block_rows)
        k = _lib.check_sparse_search(index.n, k)[0]
        idx = np.empty((hi - lo, k), dtype=np.int32)
        dist = np.empty((hi - lo, k), dtype=np.float32)
        for a, b in blocks:
            index.search(k, a, b, out=(idx[a - lo:b - lo], dist[a - lo:b - lo]))
    return lo, hi, idx, dist


def sparse_knn_target_shard(ctx, indptr, indices, values, n_features, k, rank, world, metric="cosine",
                            block_rows=None):
    """This rank's part of Context.knn_sparse on the whole CSR with the TARGETS divided: (lo, hi, idx int32 [n, k],
    dist float32 [n, k]), the k nearest rows among the rank's own rows [lo, hi) of shard_rows(n, world) for EVERY row
    of the CSR, neighbour indices global.  The rank builds the index of its own rows only (local_csr, the values
    sliced alongside) and asks it about all n rows with SparseIndex.query, in blocks of at most block_rows query rows
    (None: one block); the shard's first row is added to the indices.  merge_sparse_topk of the ranks' (idx, dist)
    is the one-GPU answer bit for bit.  No collective and no process group: a caller on several GPUs gathers the
    parts itself.  Needs k <= hi - lo on every rank that is asked (ValueError, before any GPU work); the index is
    freed before the call returns."""
    n, F = _lib.check_sparse_csr(indptr, indices, values, n_features, metric=metric)
    lo, hi, _ = sparse_rank_blocks(n, rank, world)
    k = _lib.check_sparse_search(n, k)[0]
    if k > hi - lo:
        raise ValueError("rank %d of %d holds the %d target rows [%d, %d): need k = %d <= that"
                         % (rank, world, hi - lo, lo, hi, k))
    ip, ix = local_csr(indptr, indices, lo, hi)
    vals = None if values is None else np.ascontiguousarray(values[indptr[lo]:indptr[hi]])
    with ctx.sparse_index(ip, ix, vals, F, metric=metric) as index:
        idx, dist = index.query(indptr, indices, values, k, block_rows=block_rows)
    idx += np.int32(lo)
    return lo, hi, idx, dist


def merge_sparse_topk(parts, k):
    """The k nearest targets per query over the ranks' lists: parts is a sequence of (idx int32 [nq, k_r], dist
    float32 [nq, k_r]) with k_r >= min(k, targets of that rank) and global, pairwise distinct target indices; returns
    (idx int32 [nq, k], dist float32 [nq, k]), per query the k smallest by (distance bits as uint32, index).  Plain
    numpy.

    This is exact.  Every rule of the sparse search -- the order by (distance bits, index), the distance-1 fill in
    index order, the closed form of a zero query (zero rows at 0 in index order, then the others at 1 in index order)
    -- is "the first k targets under ONE total order of the targets", the order by (distance bits, index), and a
    target's distance from a query does not depend on which other targets are indexed with it.  A rank's list is the
    first k of its own targets under that order, so every one of the first k targets overall is in its rank's list,
    and the first k of the union of the lists is the answer of the whole call bit for bit, whatever the order of the
    parts."""
    k = int(k)
    if not parts:
        raise ValueError("merge_sparse_topk needs at least one part")
    idx = np.concatenate([np.asarray(p[0], dtype=np.int32) for p in parts], axis=1)
    dist = np.concatenate([np.asarray(p[1], dtype=np.float32) for p in parts], axis=1)
    if idx.shape != dist.shape or idx.ndim != 2 or not 1 <= k <= idx.shape[1]:
        raise ValueError("parts must be (idx [nq, k_r], dist [nq, k_r]) pairs with at least k = %d columns in all" % k)
    key = (np.ascontiguousarray(dist).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint32)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(idx, order, axis=1), np.take_along_axis(dist, order, axis=1)


def sparse_radius_target_shard(ctx, indptr, indices, values, n_features, radius, rank, world, metric="cosine",
                               block_rows=None, max_hits=1 << 26):
    """This rank's part of SparseIndex.radius_search(radius) on the whole CSR with the TARGETS divided: (lo, hi, indptr
    int64 [n + 1], idx int32, dist float32), for EVERY row of the CSR the rank's own rows [lo, hi) of shard_rows(n,
    world) within `radius` of it, in (distance bits, index) order, indices global.  The rank builds the index of its
    own rows only (local_csr, the values sliced alongside) and asks it about all n rows with SparseIndex.radius_query,
    in blocks of at most block_rows query rows (None: one block), max_hits capping the hits of one device call; the
    shard's first row is added to the indices.  merge_sparse_radius of the ranks' (indptr, idx, dist) is the one-GPU
    answer bit for bit.  No collective and no process group: a caller on several GPUs gathers the parts itself.  There
    is no k, so no rank is too small to answer, but every rank that is asked needs at least one row (the index does);
    the index is freed before the call returns."""
    n, F = _lib.check_sparse_csr(indptr, indices, values, n_features, metric=metric)
    _lib.check_sparse_radius(radius, max_hits)
    lo, hi, _ = sparse_rank_blocks(n, rank, world)
    if hi == lo:
        raise ValueError("rank %d of %d holds no rows of %d: the sparse index needs at least one" % (rank, world, n))
    ip, ix = local_csr(indptr, indices, lo, hi)
    vals = None if values is None else np.ascontiguousarray(values[indptr[lo]:indptr[hi]])
    with ctx.sparse_index(ip, ix, vals, F, metric=metric) as index:
        out_ip, idx, dist = index.radius_query(indptr, indices, values, radius, block_rows=block_rows,
                                               max_hits=max_hits)
    idx += np.int32(lo)
    return lo, hi, out_ip, idx, dist


def merge_sparse_radius(parts):
    """Every target within the radius per query over the ranks' ragged rows: parts is a sequence of (indptr int64
    [nq + 1], idx int32 [indptr[-1]], dist float32 [indptr[-1]]), each rank's result for the same nq queries with
    global, pairwise distinct target indices; returns (indptr int64 [nq + 1], idx int32, dist float32), indptr the
    sum of the parts' indptrs and row q the union of the parts' rows q, ascending by (distance bits as uint32, index).
    Plain numpy.

    This is exact.  Every rule of the sparse radius search is "EVERY target whose key is within the bound, under ONE
    total order of the targets", the order by (distance bits, index): a row holds the targets at distance <= radius in
    that order, and the closed form of a zero query (zero norm, empty set, zero mass) is the index's zero rows at
    distance 0 in index order and nothing else (every other row is at 1 > radius).  A target's distance from a query
    does not depend on which other targets are indexed with it, and whether a row is a zero row is a property of the
    row alone.  So a rank's row is exactly the targets of the answer that the rank holds, each rank lists its own zero
    rows at distance 0 for a zero query, and the union of the ranks' rows in key order -- for a zero query all zero
    rows in index order -- is the row of the whole call bit for bit, whatever the order of the parts.  Equal keys in
    two parts are a duplicate index, the caller's broken promise: both come out, the earlier part's first."""
    if not parts:
        raise ValueError("merge_sparse_radius needs at least one part")
    ips = [np.asarray(p[0], dtype=np.int64) for p in parts]
    nq = ips[0].size - 1
    for ip, p in zip(ips, parts):
        if ip.ndim != 1 or ip.size != nq + 1 or ip[0] != 0 or np.any(np.diff(ip) < 0) \
                or np.size(p[1]) != ip[-1] or np.size(p[2]) != ip[-1]:
            raise ValueError("parts must be (indptr [nq + 1] from 0, never decreasing; idx [indptr[-1]]; dist "
                             "[indptr[-1]]) triples for the same nq = %d queries" % nq)
    idx = np.concatenate([np.asarray(p[1], dtype=np.int32).ravel() for p in parts])
    dist = np.concatenate([np.asarray(p[2], dtype=np.float32).ravel() for p in parts])
    query = np.concatenate([np.repeat(np.arange(nq, dtype=np.int64), np.diff(ip)) for ip in ips])
    key = (np.ascontiguousarray(dist).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint32)
    order = np.lexsort((key, query))  # (stable: equal keys of a query stay in part order)
    indptr = np.sum(ips, axis=0, dtype=np.int64)
    return indptr, idx[order], dist[order]


def sparse_shard_offsets(counts, k):
    """The ranks' row ranges [(lo, hi), ...] of a target-sharded sparse search from their row counts, in rank order
    (the counts of shard_rows give its blocks back), after the check that every rank can answer k: a rank's list
    holds k of ITS rows, so k may not exceed the smallest count.  ValueError otherwise, the same words on every rank,
    naming the first rank with the fewest rows.  Needs no GPU."""
    counts = [int(c) for c in counts]
    if not counts or min(counts) < 0:
        raise ValueError("need the row count, >= 0, of at least one rank, got %r" % (counts,))
    k = int(k)
    short = min(range(len(counts)), key=lambda r: (counts[r], r))
    if k > counts[short]:
        raise ValueError("rank %d of %d holds %d target rows: a target-sharded sparse search needs k = %d <= the rows of "
                         "every rank (use fewer ranks, a smaller k, or shard the queries instead)"
                         % (short, len(counts), counts[short], k))
    his = np.cumsum(counts).tolist()
    return [(hi - c, hi) for c, hi in zip(counts, his)]


_gloo_groups = {}  # process group (None: the default one) -> its gloo twin, created once


def _host_group(group):
    """The group the host arrays of sparse_knn_sharded travel on: `group` itself (None: the default group) when its
    backend is gloo, else a gloo group of the same ranks, created on first use and kept (every rank of the group gets
    here in the same call, as new_group requires).  Under nccl that creation is the one line of this path that a
    one-GPU rehearsal cannot run."""
    if dist.get_backend(group) == "gloo":
        return group
    if group not in _gloo_groups:
        ranks = None if group is None else dist.get_process_group_ranks(group)
        _gloo_groups[group] = dist.new_group(ranks=ranks, backend="gloo")
    return _gloo_groups[group]


def sparse_knn_sharded(ctx, indptr_local, indices_local, values_local, n_features, k, metric="cosine", group=None,
                       block_rows=None):
    """Context.knn_sparse over the ranks of a process group with the TARGETS divided, collective included: every rank
    calls this with ITS rows only (a CSR with indptr rebased to 0, values alongside or None; the ranks' blocks, in rank
    order, are the whole matrix) and gets (lo, hi, idx int32 [hi - lo, k], dist float32 [hi - lo, k]): the rows
    [lo, hi) of knn_sparse on the concatenated CSR bit for bit, neighbour indices global.

    Rounds.  (1) One all-gather of (rows, stored entries, values given?) per rank: every rank knows every lo.  (2)
    sparse_shard_offsets: k above the smallest rank's rows is the same ValueError on every rank, before any GPU work.
    (3) Each rank builds the index of its own rows.  (4) For each source rank s in turn: s broadcasts its block (indptr,
    indices, and values unless they are None), every rank asks its index about the block (SparseIndex.query in blocks of
    block_rows rows) and adds its own lo to the indices, and the [rows_s, k] lists are gathered to s into one part-major
    buffer [world, rows_s, k], which is what fdr_topk_merge takes: nothing is transposed.  (5) The index is freed; each
    rank merges its buffer on its GPU (Context.topk_merge, exact: merge_sparse_topk's docstring), all ranks at once.

    A rank holds on the host its own block, one foreign block, a foreign block's k lists, and world x k candidates for
    each of its own rows; never the whole CSR, never [n, k].  On the device it holds 1 / world of the index.  Every
    rank sees every query: the posting walk is divided by the ranks, the upload of the queries is not.

    The arrays are host arrays on both ends (the sparse API takes host pointers), so the exchange runs on a gloo group:
    `group` (None: the default group) when that is gloo, else a gloo group of the same ranks created once.  Without an
    initialised process group the call is the one-rank case.  sparse_knn_rank is the alternative that replicates the
    index and exchanges nothing."""
    _lib.sparse_metric_code(metric)
    # (a rank without rows gets as far as the k check, which every rank fails together)
    n_loc, _, F = _lib._check_sparse(indptr_local, indices_local, values_local, n_features, None, metric, min_rows=0)
    multi = dist.is_initialized()
    g = _host_group(group) if multi else None
    rank, world = (dist.get_rank(g), dist.get_world_size(g)) if multi else (0, 1)
    src = (lambda s: s if g is None else dist.get_global_rank(g, s))
    # (1) the row counts
    mine = torch.tensor([n_loc, indices_local.size, 0 if values_local is None else 1], dtype=torch.int64)
    every = [torch.empty_like(mine) for _ in range(world)]
    if multi:
        dist.all_gather(every, mine, group=g)
    else:
        every = [mine]
    rows, nnz, has_values = (tuple(int(t[c]) for t in every) for c in range(3))
    if len(set(has_values)) != 1:
        raise ValueError("the ranks disagree on whether the rows carry values: %r" % (has_values,))
    # (2) k against the smallest shard, before any GPU work
    blocks = sparse_shard_offsets(rows, k)
    lo, hi = blocks[rank]
    if hi > np.iinfo(np.int32).max:
        raise ValueError("need fewer than 2^31 rows in all")
    k = _lib.check_sparse_search(n_loc, k)[0]
    idx_parts = np.empty((world, n_loc, k), dtype=np.int32)  # the gather's receive buffers, part-major
    dist_parts = np.empty((world, n_loc, k), dtype=np.float32)
    # (3), (4)
    with ctx.sparse_index(indptr_local, indices_local, values_local, F, metric=metric) as index:
        for s in range(world):
            if s == rank:
                ip, ix, vals = indptr_local, indices_local, values_local
            else:
                ip = np.empty(rows[s] + 1, dtype=np.int64)
                ix = np.empty(nnz[s], dtype=np.int32)
                vals = np.empty(nnz[s], dtype=np.float32) if has_values[s] else None
            if multi:
                dist.broadcast(torch.from_numpy(ip), src(s), group=g)
                if nnz[s]:
                    dist.broadcast(torch.from_numpy(ix), src(s), group=g)
                    if vals is not None:
                        dist.broadcast(torch.from_numpy(vals), src(s), group=g)
            out = (idx_parts[rank], dist_parts[rank]) if s == rank else None  # (the owner's own part is in place)
            qi, qd = index.query(ip, ix, vals, k, out=out, block_rows=block_rows)
            qi += np.int32(lo)
            if multi:
                for part, buf in ((qi, idx_parts), (qd, dist_parts)):
                    dist.gather(torch.from_numpy(part), list(torch.from_numpy(buf).unbind(0)) if s == rank else None,
                                dst=src(s), group=g)
            del ip, ix, vals, qi, qd
    # (5) the index is freed; every rank merges its own rows' lists
    idx, dst = ctx.topk_merge(idx_parts, dist_parts, k)
    return lo, hi, idx, dst


def sparse_radius_offsets(counts):
    """The ranks' row ranges [(lo, hi), ...] of a target-sharded sparse radius search from their row counts, in rank
    order.  There is no k, so no rank is too small to answer; but the sparse index needs at least one row
    (Context.sparse_index refuses an empty CSR), so a rank without rows is a ValueError, the same words on every rank,
    naming the first such rank.  Needs no GPU."""
    counts = [int(c) for c in counts]
    if not counts or min(counts) < 0:
        raise ValueError("need the row count, >= 0, of at least one rank, got %r" % (counts,))
    if min(counts) == 0:
        raise ValueError("rank %d of %d holds no rows: a rank of a target-sharded sparse radius search builds the "
                         "index of its own rows, and the sparse index needs at least one row (use fewer ranks)"
                         % (counts.index(0), len(counts)))
    his = np.cumsum(counts).tolist()
    if his[-1] > np.iinfo(np.int32).max:
        raise ValueError("need fewer than 2^31 rows in all")
    return [(hi - c, hi) for c, hi in zip(counts, his)]


def sparse_radius_sharded(ctx, indptr_local, indices_local, values_local, n_features, radius, metric="cosine",
                          group=None, block_rows=None, max_hits=1 << 26):
    """SparseIndex.radius_search(radius) of the whole CSR over the ranks of a process group with the TARGETS divided,
    collective included: every rank calls this with ITS rows only (as in sparse_knn_sharded) and gets (lo, hi, indptr
    int64 [hi - lo + 1], idx int32, dist float32): the rows [lo, hi) of the one-GPU radius search on the concatenated
    CSR bit for bit, every row within `radius` in (distance bits, index) order, self among them, indices global.

    Rounds, those of sparse_knn_sharded.  (1) One all-gather of (rows, stored entries, values given?) per rank.  (2)
    The checks, before any GPU work and with the same ValueError on every rank: radius and max_hits
    (_lib.check_sparse_radius), and sparse_radius_offsets: there is no k and so no k <= smallest-shard condition, but
    a rank with 0 rows is refused, because the sparse index cannot be built of no rows.  (3) Each rank builds the index
    of its own rows.  (4) For each source rank s in turn: s broadcasts its block, every rank asks its index about it
    (SparseIndex.radius_query in blocks of block_rows rows, max_hits capping the hits of one device call) and adds its
    own lo to the indices; the indptrs, of the fixed shape [rows_s + 1], are gathered to s; the ragged payloads follow
    point to point (a gather needs equal shapes): every other rank sends its indices, then its distances, and s posts
    receives of the lengths the indptrs state, rank after rank; an empty payload is not sent.  (5) The index is freed;
    each rank merges the world's rows of its own queries on its GPU (Context.radius_merge with max_entries = max_hits,
    exact: merge_sparse_radius's docstring), all ranks at once.

    A rank holds on the host its own block, one foreign block, its answer to a foreign block, and, for its own rows,
    every rank's hits once as parts and once merged (8 bytes per hit each); never the whole CSR.  On the device it
    holds 1 / world of the index, one call's hits (max_hits x 16 bytes), and for the merge 16 bytes per entry of a
    piece.  One row with more than max_hits hits over all ranks is a ValueError of the merge.  Every rank sees every
    query: the posting walk is divided by the ranks, the upload of the queries is not.  The exchange runs on a gloo
    group as in sparse_knn_sharded; without an initialised process group the call is the one-rank case."""
    _lib.sparse_metric_code(metric)
    n_loc, _, F = _lib._check_sparse(indptr_local, indices_local, values_local, n_features, None, metric, min_rows=0)
    multi = dist.is_initialized()
    g = _host_group(group) if multi else None
    rank, world = (dist.get_rank(g), dist.get_world_size(g)) if multi else (0, 1)
    src = (lambda s: s if g is None else dist.get_global_rank(g, s))
    # (1) the row counts
    mine = torch.tensor([n_loc, indices_local.size, 0 if values_local is None else 1], dtype=torch.int64)
    every = [torch.empty_like(mine) for _ in range(world)]
    if multi:
        dist.all_gather(every, mine, group=g)
    else:
        every = [mine]
    rows, nnz, has_values = (tuple(int(t[c]) for t in every) for c in range(3))
    if len(set(has_values)) != 1:
        raise ValueError("the ranks disagree on whether the rows carry values: %r" % (has_values,))
    # (2) the radius, the cap and the row counts, before any GPU work
    _lib.check_sparse_radius(radius, max_hits)
    _lib._check_block_rows(block_rows)
    lo, hi = sparse_radius_offsets(rows)[rank]
    parts = [None] * world  # per source rank of the answers to MY rows: (indptr, idx, dist)
    # (3), (4)
    with ctx.sparse_index(indptr_local, indices_local, values_local, F, metric=metric) as index:
        for s in range(world):
            if s == rank:
                ip, ix, vals = indptr_local, indices_local, values_local
            else:
                ip = np.empty(rows[s] + 1, dtype=np.int64)
                ix = np.empty(nnz[s], dtype=np.int32)
                vals = np.empty(nnz[s], dtype=np.float32) if has_values[s] else None
            if multi:
                dist.broadcast(torch.from_numpy(ip), src(s), group=g)
                if nnz[s]:
                    dist.broadcast(torch.from_numpy(ix), src(s), group=g)
                    if vals is not None:
                        dist.broadcast(torch.from_numpy(vals), src(s), group=g)
            qp, qi, qd = index.radius_query(ip, ix, vals, radius, block_rows=block_rows, max_hits=max_hits)
            qi += np.int32(lo)
            if s == rank:
                parts[rank] = (qp, qi, qd)
            if multi:
                ips = np.empty((world, rows[s] + 1), dtype=np.int64) if s == rank else None
                dist.gather(torch.from_numpy(qp), list(torch.from_numpy(ips).unbind(0)) if s == rank else None,
                            dst=src(s), group=g)
                if s == rank:
                    for r in range(world):
                        if r == rank:
                            continue
                        ri = np.empty(int(ips[r, -1]), dtype=np.int32)
                        rd = np.empty(int(ips[r, -1]), dtype=np.float32)
                        if ri.size:
                            dist.recv(torch.from_numpy(ri), src=src(r), group=g)
                            dist.recv(torch.from_numpy(rd), src=src(r), group=g)
                        parts[r] = (ips[r].copy(), ri, rd)
                elif qi.size:
                    dist.send(torch.from_numpy(qi), dst=src(s), group=g)
                    dist.send(torch.from_numpy(qd), dst=src(s), group=g)
            del ip, ix, vals, qp, qi, qd
    # (5) the index is freed; every rank merges its own rows' lists
    indptr, idx, dst = ctx.radius_merge(parts, max_entries=max_hits)
    return lo, hi, indptr, idx, dst


def local_csr(indptr, indices, lo, hi):
    """Rows [lo, hi) of a host CSR, indptr rebased to 0 (numpy)."""
    ip = np.ascontiguousarray(indptr[lo:hi + 1] - indptr[lo], dtype=np.int64)
    ix = np.ascontiguousarray(indices[indptr[lo]:indptr[hi]], dtype=np.int32)
    return ip, ix
