// Part of libfedrann_hip.so (included by fedrann_hip.hip, behind graph_symmetrize.inc).
//
// fdr_graph_expand: the candidate generator of a neighbour-list refinement (NN-descent's local join, without its
// flags and sampling): the distinct rows within two hops of every row of a block.  The graph is fdr_graph_symmetrize's:
// square on n rows, ragged, rows in any order.  N_f(x) is the first min(fan, len(x)) entries of row x in ascending order
// of key = distance bits << 32 | index.  Row r of the result, q_lo <= r < q_lo + nq, holds s iff
//     s is in N_f(r), or
//     s != r and s is in N_f(t) for some t in N_f(r),
// strictly ascending by index, every index once: a function of the input alone, at most fan + fan^2 entries a row.  A
// read's own index stays exactly when the read lists itself inside its fan, so whatever convention the search had
// survives.  An index listed twice in a row is NOT refused here: it takes two places of the fan cut and comes out once.
// fedrann_amd.graph.expand_rows is the model of this file, bit for bit, and the route without a GPU.
//
// E1  ge_pack_kernel, one thread per entry of the WHOLE graph (any row can be some t): the entry's row (a binary search
//     in the indptr), the index and distance rules into the refusal record (gs_refuse: the smallest row << 8 | rule), the
//     key.  rocprim::segmented_radix_sort_keys over the input rows: the fan cut is then a prefix of each row.
// E2  ge_bound_kernel, one thread per row of the block: bound[r] = |N_f(r)| + sum over t in N_f(r) of |N_f(t)|, and the
//     scan.  The host reads the total and the refusal record here, before anything is written to indptr_out.
// E3  ge_gather_kernel, one wave per row of the block: the one-hop indices at the head of the row's segment, then
//     N_f(t) for every t in turn, consecutive lanes on consecutive entries; a two-hop s == r is written as GE_NONE (no
//     index: n < 2^31), which sorts behind every index.
// E4  rocprim::segmented_radix_sort_keys of the 32-bit indices over the bound's segments.
// E5  ge_heads_kernel, one wave per row: the first entry of every run of equal indices, GE_NONE apart, is marked.  The
//     exclusive scan of the marks over ALL bound entries is every marked entry's place in the result (the segments lie
//     in row order), and off[r] = scan[boff[r]] is the result's row pointer: the exact prefix sums, without an atomic,
//     so there is no cursor to cross-check and the order inside a row is the sort's.
// E6  ge_compact_kernel, one thread per bound entry: a marked entry goes to its place.
//
// Device bytes: 24 per input entry (GraphSymScratch: index 4, distance 4, packed key 8, ordered key 8), 12 per bound
// entry (gathered index / mark 4, sorted index 4, scan 4), 4 per result entry, 8 per row of the graph (the indptr) and
// 24 per row of the block (bound, its scan, the result's row pointer), beside rocprim's temporary storage.
// Bounds: the host has checked the indptr (starts at 0, never decreases, totals below 2^31) before the upload.  E2 uses
// t only when 0 <= t < n, whatever the entry holds; E3 .. E6 run only after the host has read an empty refusal record
// and a bound total below 2^31.  Every store of E3 is checked against the end of its row's segment and every store of
// E6 against the result's total; one that falls outside is counted and the call fails as an internal error.
// The held symmetrised graph (gs.rr), the indexes and the re-score rows are not touched.

constexpr unsigned GE_NONE = 0xffffffffu;
constexpr int GE_WAVES = 4;  // rows of the block per workgroup of E3 and E5

__global__ __launch_bounds__(256) void ge_pack_kernel(long long total, long long n, const long long *__restrict__ indptr,
                                                      const int *__restrict__ idx, const float *__restrict__ dist,
                                                      u64 *__restrict__ packed, u64 *__restrict__ refusal) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    u64 bad = TM_NONE;
    if (i < total) {
        long long lo = 0, hi = n;  // the r in [0, n) with indptr[r] <= i < indptr[r + 1]  (as gs_pack_kernel)
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (indptr[mid] <= i) lo = mid;
            else hi = mid;
        }
        const int t = idx[i];
        const unsigned bits = __float_as_uint(dist[i]);
        packed[i] = ((u64)bits << 32) | (u64)(unsigned)t;
        int rule = 0;
        if (t < 0 || (long long)t >= n) rule = GS_RULE_INDEX;
        else if (bits > 0x7f800000u) rule = GS_RULE_DISTANCE;
        if (rule) bad = ((u64)lo << 8) | (u64)rule;
    }
    gs_refuse(bad, refusal);
}

// |N_f(x)| of a row x in [0, n)
__device__ __forceinline__ int ge_fan_len(const long long *__restrict__ indptr, long long x, int fan) {
    return (int)min((long long)fan, indptr[x + 1] - indptr[x]);
}

// one thread per element of bound: nq rows and the 0 behind them
__global__ __launch_bounds__(256) void ge_bound_kernel(long long n, int fan, long long q_lo, long long nq,
                                                       const long long *__restrict__ indptr,
                                                       const u64 *__restrict__ bykey, long long *__restrict__ bound) {
    const long long rq = (long long)blockIdx.x * 256 + threadIdx.x;
    if (rq > nq) return;
    long long sum = 0;
    if (rq < nq) {
        const long long r = q_lo + rq, b = indptr[r];
        const int f = ge_fan_len(indptr, r, fan);
        sum = f;
        for (int j = 0; j < f; ++j) {
            const long long t = (long long)(unsigned)bykey[b + j];
            if (t < n) sum += ge_fan_len(indptr, t, fan);  // (E1 refuses every other entry; the test keeps the load inside)
        }
    }
    bound[rq] = sum;
}

__global__ __launch_bounds__(64 * GE_WAVES) void ge_gather_kernel(long long n, int fan, long long q_lo, long long nq,
                                                                  const long long *__restrict__ indptr,
                                                                  const u64 *__restrict__ bykey,
                                                                  const long long *__restrict__ boff,
                                                                  unsigned *__restrict__ cand, u64 *__restrict__ flags) {
    __shared__ int tl[GE_WAVES][FDR_MAX_K], ts[GE_WAVES][FDR_MAX_K], tm[GE_WAVES][FDR_MAX_K], tp[GE_WAVES][FDR_MAX_K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long rq = (long long)blockIdx.x * GE_WAVES + w;
    const bool live = rq < nq;
    const long long r = q_lo + rq;
    long long seg0 = 0, seg1 = 0;
    int f = 0;
    if (live) {
        seg0 = boff[rq];
        seg1 = boff[rq + 1];
        f = ge_fan_len(indptr, r, fan);
    }
    auto place = [&](long long pos, unsigned v) {
        if (pos < seg1) cand[pos] = v;
        else atomicAdd(flags, 1ull);
    };
    // the row's fan: t, where N_f(t) starts, its length, and the lengths' exclusive scan (two halves of 64)
    int carry = 0;
    for (int h = 0; h < FDR_MAX_K; h += 64) {  // (wave-uniform trips: the shuffles see every lane)
        const int j = h + lane;
        long long t = -1;
        int m = 0, start = 0;
        if (j < f) {
            t = (long long)(unsigned)bykey[indptr[r] + j];
            if (t < n) {
                start = (int)indptr[t];  // (fewer than 2^31 entries)
                m = ge_fan_len(indptr, t, fan);
            }
            place(seg0 + j, (unsigned)t);  // one hop: the row's own entries, its own index among them where listed
        }
        int incl = m;
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        tl[w][j] = (int)t;
        ts[w][j] = start;
        tm[w][j] = m;
        tp[w][j] = carry + incl - m;
        carry += __shfl(incl, 63, 64);
    }
    __syncthreads();
    // two hops: N_f(t) for every t of the fan in turn
    for (int j = 0; j < f; ++j) {
        const int m = tm[w][j];
        const long long from = ts[w][j], to = seg0 + f + tp[w][j];
        for (int l = lane; l < m; l += 64) {
            const unsigned s = (unsigned)bykey[from + l];
            place(to + l, (long long)s == r ? GE_NONE : s);
        }
    }
}

// head[i] = 1 where sorted[i] opens a run of its segment and is an index, else 0; head[B] = 0
__global__ __launch_bounds__(64 * GE_WAVES) void ge_heads_kernel(long long nq, const long long *__restrict__ boff,
                                                                 const unsigned *__restrict__ sorted,
                                                                 unsigned *__restrict__ head) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long rq = (long long)blockIdx.x * GE_WAVES + w;
    if (rq > nq) return;
    if (rq == nq) {
        if (lane == 0) head[boff[nq]] = 0u;
        return;
    }
    const long long seg0 = boff[rq], seg1 = boff[rq + 1];
    for (long long i = seg0 + lane; i < seg1; i += 64) {
        const unsigned v = sorted[i];
        head[i] = v != GE_NONE && (i == seg0 || sorted[i - 1] != v) ? 1u : 0u;
    }
}

// off[r] = scan[boff[r]] for the nq rows and the total behind them
__global__ __launch_bounds__(256) void ge_rowptr_kernel(long long nq, const long long *__restrict__ boff,
                                                        const unsigned *__restrict__ scan, long long *__restrict__ off) {
    const long long rq = (long long)blockIdx.x * 256 + threadIdx.x;
    if (rq <= nq) off[rq] = (long long)scan[boff[rq]];
}

__global__ __launch_bounds__(256) void ge_compact_kernel(long long B, long long total, const unsigned *__restrict__ head,
                                                         const unsigned *__restrict__ scan,
                                                         const unsigned *__restrict__ sorted, int *__restrict__ out,
                                                         u64 *__restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B || !head[i]) return;
    const long long pos = scan[i];
    if (pos < total) out[pos] = (int)sorted[i];
    else atomicAdd(flags, 1ull);
}

FDR_EXPORT int fdr_graph_expand(fdr_ctx *ctx, int64_t n, const int64_t *indptr, const int32_t *idx, const float *dist,
                                int32_t fan, int64_t q_lo, int64_t nq, int64_t max_entries, int64_t *indptr_out) {
    static const char who[] = "graph_expand";
    int rc = use_device(ctx);
    if (rc) return rc;
    GraphSymScratch &gs = ctx->gs;
    GraphExpandScratch &ge = ctx->ge;
    ge.drop();
    if (fan < 1 || fan > FDR_MAX_K) return fail(FDR_E_ARG, "%s: fan=%d unsupported (1..%d)", who, fan, FDR_MAX_K);
    if (n < 1 || n > INT32_MAX) return fail(FDR_E_ARG, "%s: n (%lld) must be in [1, 2^31)", who, (long long)n);
    if (q_lo < 0 || nq < 0 || q_lo > n || nq > n - q_lo)
        return fail(FDR_E_ARG, "%s: rows [%lld, %lld + %lld) are no range of the %lld rows", who, (long long)q_lo,
                    (long long)q_lo, (long long)nq, (long long)n);
    if (max_entries < 1 || max_entries > INT32_MAX)
        return fail(FDR_E_ARG, "%s: max_entries (%lld) must be in [1, 2^31)", who, (long long)max_entries);
    if (!indptr || !indptr_out) return fail(FDR_E_ARG, "%s: null indptr pointer", who);
    if ((rc = gs_check_indptr(who, n, indptr))) return rc;
    const long long total = indptr[n];
    if (total > 0 && (!idx || !dist)) return fail(FDR_E_ARG, "%s: null pointer", who);
    const size_t rows = (size_t)nq + 1;
    auto hold_empty = [&]() {  // (no row, or no entry: an empty result, held)
        for (size_t r = 0; r < rows; ++r) indptr_out[r] = 0;
        ge.h_off.assign(rows, 0ll);
        ge.n = n;
        ge.q_lo = q_lo;
        ge.nq = nq;
        ge.held = 0;
        return FDR_OK;
    };
    if (total == 0) return hold_empty();
    const hipStream_t st = ctx->stream;
    const dim3 block(256);
    // E1: the whole graph, its check, every row ordered by key
    if ((rc = gs.indptr.reserve((size_t)n + 1))) return rc;
    if ((rc = gs.idx.reserve((size_t)total))) return rc;
    if ((rc = gs.dist.reserve((size_t)total))) return rc;
    if ((rc = gs.packed.reserve((size_t)total))) return rc;
    if ((rc = gs.byidx.reserve((size_t)total))) return rc;
    if ((rc = gs.refusal.reserve(1))) return rc;
    if ((rc = ge.bound.reserve(rows))) return rc;
    if ((rc = ge.boff.reserve(rows))) return rc;
    if ((rc = ge.off.reserve(rows))) return rc;
    if ((rc = ge.flags.reserve(1))) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "the caller's indptr is the device's");
    HIP_TRY(upload(gs.indptr, reinterpret_cast<const long long *>(indptr), (size_t)n + 1, st));
    HIP_TRY(upload(gs.idx, idx, (size_t)total, st));
    HIP_TRY(upload(gs.dist, dist, (size_t)total, st));
    HIP_TRY(hipMemsetAsync(gs.refusal.ptr(), 0xff, 8, st));
    HIP_TRY(hipMemsetAsync(ge.flags.ptr(), 0, 8, st));
    hipLaunchKernelGGL(ge_pack_kernel, dim3((unsigned)((total + 255) / 256)), block, 0, st, total, (long long)n,
                       gs.indptr.ptr(), gs.idx.ptr(), gs.dist.ptr(), gs.packed.ptr(), gs.refusal.ptr());
    HIP_TRY(hipGetLastError());
    const u64 *bykey = gs.byidx.ptr();  // (the array's name is the symmetrise's: here every row is ordered by key)
    auto by_key = [&](void *tmp, size_t &bytes) {  // (all 64 bits: a refused entry's key may have any of them set)
        return rocprim::segmented_radix_sort_keys(tmp, bytes, gs.packed.ptr(), gs.byidx.ptr(), (unsigned)total, (unsigned)n,
                                                  gs.indptr.ptr(), gs.indptr.ptr() + 1, 0, 64, st);
    };
    if ((rc = rocprim_run(gs.tmp, "rocprim::segmented_radix_sort_keys", by_key))) return rc;
    // E2, the refusal record, the bound
    hipLaunchKernelGGL(ge_bound_kernel, dim3((unsigned)(nq / 256 + 1)), block, 0, st, (long long)n, (int)fan,
                       (long long)q_lo, (long long)nq, gs.indptr.ptr(), bykey, ge.bound.ptr());
    HIP_TRY(hipGetLastError());
    auto scan_bound = [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, ge.bound.ptr(), ge.boff.ptr(), 0ll, rows, rocprim::plus<long long>(), st);
    };
    if ((rc = rocprim_run(gs.tmp, "rocprim::exclusive_scan", scan_bound))) return rc;
    u64 refused = TM_NONE;
    long long B = 0;
    HIP_TRY(download(&refused, gs.refusal, 1, st));
    HIP_TRY(hipMemcpyAsync(&B, ge.boff.ptr() + nq, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (refused != TM_NONE) return gs_refused(who, refused);  // (nothing has been written to indptr_out)
    if (B > INT32_MAX)
        return fail(FDR_E_ARG, "%s: the rows [%lld, %lld) have %lld entries within two hops before duplicates go, 2^31 "
                    "or more: take fewer rows a call", who, (long long)q_lo, (long long)(q_lo + nq), B);
    if (B == 0) return hold_empty();
    // E3, E4
    if ((rc = ge.cand.reserve((size_t)B + 1))) return rc;
    if ((rc = ge.sorted.reserve((size_t)B))) return rc;
    if ((rc = ge.pos.reserve((size_t)B + 1))) return rc;
    const dim3 per_wave((unsigned)((nq + 1 + GE_WAVES - 1) / GE_WAVES)), wave_block(64 * GE_WAVES);
    hipLaunchKernelGGL(ge_gather_kernel, per_wave, wave_block, 0, st, (long long)n, (int)fan, (long long)q_lo,
                       (long long)nq, gs.indptr.ptr(), bykey, ge.boff.ptr(), ge.cand.ptr(), ge.flags.ptr());
    HIP_TRY(hipGetLastError());
    auto by_index = [&](void *tmp, size_t &bytes) {
        return rocprim::segmented_radix_sort_keys(tmp, bytes, ge.cand.ptr(), ge.sorted.ptr(), (unsigned)B, (unsigned)nq,
                                                  ge.boff.ptr(), ge.boff.ptr() + 1, 0, 32, st);
    };
    if ((rc = rocprim_run(gs.tmp, "rocprim::segmented_radix_sort_keys", by_index))) return rc;
    // E5: the run heads (in cand, which the sort has read), their scan, the result's row pointer, the cap
    hipLaunchKernelGGL(ge_heads_kernel, per_wave, wave_block, 0, st, (long long)nq, ge.boff.ptr(), ge.sorted.ptr(),
                       ge.cand.ptr());
    HIP_TRY(hipGetLastError());
    auto scan_heads = [&](void *tmp, size_t &bytes) {  // (at most B < 2^31 heads)
        return rocprim::exclusive_scan(tmp, bytes, ge.cand.ptr(), ge.pos.ptr(), 0u, (size_t)B + 1, rocprim::plus<unsigned>(),
                                       st);
    };
    if ((rc = rocprim_run(gs.tmp, "rocprim::exclusive_scan", scan_heads))) return rc;
    hipLaunchKernelGGL(ge_rowptr_kernel, dim3((unsigned)(nq / 256 + 1)), block, 0, st, (long long)nq, ge.boff.ptr(),
                       ge.pos.ptr(), ge.off.ptr());
    HIP_TRY(hipGetLastError());
    ge.h_off.resize(rows);
    HIP_TRY(download(ge.h_off.data(), ge.off, rows, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t r = 0; r < rows; ++r) indptr_out[r] = ge.h_off[r];
    const long long out = ge.h_off[nq];
    if (out > max_entries)  // (the one refusal that has written its output, as the radius searches')
        return fail(FDR_E_ARG, "%s: %lld entries exceed max_entries = %lld (indptr_out holds the counts)", who, out,
                    (long long)max_entries);
    // E6
    if ((rc = ge.out.reserve((size_t)out))) return rc;
    hipLaunchKernelGGL(ge_compact_kernel, dim3((unsigned)((B + 255) / 256)), block, 0, st, B, out, ge.cand.ptr(),
                       ge.pos.ptr(), ge.sorted.ptr(), ge.out.ptr(), ge.flags.ptr());
    HIP_TRY(hipGetLastError());
    u64 outside = 0;
    HIP_TRY(download(&outside, ge.flags, 1, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (outside != 0)
        return fail(FDR_E_HIP, "internal: %s: %llu stores fell outside their segments", who, (unsigned long long)outside);
    ge.n = n;
    ge.q_lo = q_lo;
    ge.nq = nq;
    ge.held = out;
    return FDR_OK;
}

FDR_EXPORT int fdr_graph_expand_fetch(fdr_ctx *ctx, int64_t entries, int32_t *idx_out) {
    static const char who[] = "graph_expand_fetch";
    if (int rc = use_device(ctx)) return rc;
    const GraphExpandScratch &ge = ctx->ge;
    if (ge.held < 0)
        return fail(FDR_E_STATE, "%s: the context holds no expansion (the next fdr_graph_expand and fdr_graph_free drop "
                    "it)", who);
    if (entries != ge.held)
        return fail(FDR_E_ARG, "%s: entries = %lld, the held result has %lld", who, (long long)entries, ge.held);
    if (entries == 0) return FDR_OK;
    if (!idx_out) return fail(FDR_E_ARG, "%s: null pointer", who);
    static_assert(sizeof(int) == sizeof(int32_t), "the caller's indices are the device's");
    HIP_TRY(download(reinterpret_cast<int *>(idx_out), ge.out, (size_t)entries, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FDR_OK;
}
