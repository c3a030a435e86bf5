// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit) behind knn_radius_common.inc.
// ------------------------------------------------------------------------------------------
// R1 .. R3  radius search on the sparse index (fdr_sparse_index_radius_search / _query / _fetch): every index row
// within a distance bound r of each query, 0 <= r < 1, under the index's metric.
//
// S3 / S3r (knn_sparse.inc) build, per query, the table of EVERY target at distance < 1 with its exact accumulator,
// and keep k of them.  A radius search keeps every row of that table with dist <= r; every row outside the table is
// at exactly 1.0f, so a bound below 1 never needs one.  The table walk (sp_walk) and the distance formation
// (sp_slot_dist) are the k-NN kernel's own device functions, so a pair has the same distance bits on either path
// and the comparison dist <= r is made on the float32 a k-NN search reports.  The protocol around the passes (the
// scan, the cap, the zero rows' list, the cross-check, the held result) is knn_radius_common.inc's; the counts are hit
// counts, so their scan is the result's indptr.
//   R1 sp_radius_kernel<RANGE, false>  the COUNT pass.  One wave per query, as S3: walk, then count the table's keys
//                          with dist <= r into count[q].  A query whose table would pass SP_LIMIT goes to the heavy
//                          list, as in S3, and the range form (RANGE, as S3r) adds up the counts of its ranges.  A
//                          zero (empty, zero-mass) query counts the index's zero rows.
//   R2 sp_radius_kernel<RANGE, true>   the EMIT pass repeats the walk.  A query that is not heavy holds at most
//                          SP_LIMIT + 64 table entries: its hits, as keys, are sorted in LDS by S3's bitonic network
//                          and written to its segment.  A heavy query writes each range's hits at a running offset
//                          inside its segment; the heavy segments (up to n hits each, far more than LDS holds) are
//                          then put in order by ONE rocprim segmented radix sort over them alone.
//                          R1 marks each query it hands on in handed[], and R2 leaves a marked query to its range
//                          form without walking it: a heavy query is walked to its overflow point once (R1), then
//                          once per pass in the range form.
//   R3 radius_split_kernel<false>  keys -> idx / dist, the arrays fdr_sparse_index_radius_fetch copies.
// Memory: 17 bytes per counted query, and per hit 8 bytes of sorted keys plus the 8 bytes that hold the heavy
// queries' unsorted keys first and the result afterwards.
// Cost model: two walks, so about twice the pair updates of a k-NN search of the same queries (sum over features of
// df_f^2 each), without S3's distance-1 fill; a heavy query adds R1's walk up to its overflow point and the radix
// sort of its hits.
// ------------------------------------------------------------------------------------------

// R1 (EMIT = false) and R2 (EMIT = true); the queries, the target side and the metric as in knn_sparse_kernel.
// count [nq]: R1's result (R1 of the heavy list overwrites the heavy queries' entries); off [nq + 1]: its scan, the
// segment of query q is keys_out[off[q - q0], off[q - q0 + 1]).  nzero / zlist: the index's zero rows.  handed [nq]:
// set by R1 for the queries it hands to the range form, read by R2.
template <bool RANGE, bool EMIT, int METRIC>
__global__ __launch_bounds__(64) void sp_radius_kernel(long long n, long long q0, const SpQuerySide qs,
                                                       const long long *__restrict__ runptr,
                                                       const int *__restrict__ prow, const float *__restrict__ pval,
                                                       const int *__restrict__ t_asize,
                                                       const float *__restrict__ t_mass, float radius, long long nzero,
                                                       const int *__restrict__ zlist, u64 *__restrict__ cnt,
                                                       long long *__restrict__ count,
                                                       unsigned char *__restrict__ handed,
                                                       const long long *__restrict__ off, u64 *__restrict__ keys_out,
                                                       u64 *__restrict__ flags) {
    __shared__ u64 buf[SP_CAP];  // the table, then the sort buffer
    constexpr bool JAC = METRIC == FDR_METRIC_JACCARD;
    constexpr bool WJ = METRIC == FDR_METRIC_WEIGHTED_JACCARD;
    const int lane = threadIdx.x;
    const long long q = RANGE ? (long long)qs.heavy[blockIdx.x] : q0 + (long long)blockIdx.x;
    const long long row = q - q0;
    const long long seg0 = EMIT ? off[row] : 0, seg = EMIT ? off[row + 1] - seg0 : 0;  // the segment and its length
    if (!RANGE && qs.zero[q]) {
        if (!EMIT) {
            if (lane == 0) count[row] = nzero;
        } else {
            radius_emit_zero(lane, seg0, seg, nzero, zlist, keys_out, flags);
        }
        return;
    }
    if (!RANGE && EMIT && handed[row]) return;  // (the range form's)
    const long long qb = qs.indptr[q], qe = qs.indptr[q + 1];
    const int qa = JAC ? qs.asize[q] : 0;  // |S_q|
    const double qm = WJ ? (double)qs.mass[q] : 0.0;  // A_q
    const long long nranges = RANGE ? (n + SP_W - 1) / SP_W : 1;
    const u64 lt = (1ull << lane) - 1ull;
    long long hits = 0;  // hits so far (wave-uniform)
    for (long long r = 0; r < nranges; ++r) {
        const int lo = RANGE ? (int)(r * SP_W) : 0;
        const int hi = RANGE ? (int)min(n, (long long)lo + SP_W) : (int)n;
        const bool overflow = sp_walk<RANGE, METRIC>(buf, runptr, prow, pval, qs.efeat, qs.xhat, qb, qe, lo, hi, lane);
        if (overflow) {  // (R1 alone: R2 has skipped the queries R1 handed on, and a range's table does not overflow)
            if (!EMIT && lane == 0) {
                qs.heavy[atomicAdd(&cnt[SP_CNT_HEAVY], 1ull)] = (int)q;
                handed[row] = 1;
            } else if (EMIT && lane == 0) {
                atomicAdd(&flags[RR_FLAG_MISMATCH], 1ull);
            }
            return;
        }
        u64 cand[SP_CAP / 64];  // the table's keys with dist <= r
#pragma unroll
        for (int i = 0; i < SP_CAP / 64; ++i) {
            const u64 w = buf[lane + 64 * i];
            const int t = (int)(unsigned)w;
            u64 key = KEY_INF;
            if (t != SP_EMPTY) {
                const float d = sp_slot_dist<METRIC>(w, t, qa, qm, t_asize, t_mass);
                if (d <= radius) key = ((u64)__float_as_uint(d) << 32) | (unsigned)t;
            }
            cand[i] = key;
        }
        __syncthreads();  // (the table is read: the sort buffer, or the next range's table, may take its place)
        int m = 0;
#pragma unroll
        for (int i = 0; i < SP_CAP / 64; ++i) {
            const bool h = cand[i] != KEY_INF;
            const u64 bal = __ballot(h);
            if (EMIT && h) {
                const long long at = hits + m + __popcll(bal & lt);
                if (RANGE) {
                    if (at < seg) keys_out[seg0 + at] = cand[i];
                } else {
                    buf[at] = cand[i];  // (at most SP_LIMIT + 64 < SP_CAP table entries)
                }
            }
            m += __popcll(bal);
        }
        if (EMIT && !RANGE) {
            int P = 64;
            while (P < m) P <<= 1;
            for (int i = m + lane; i < P; i += 64) buf[i] = KEY_INF;
            __syncthreads();
            sp_bitonic(buf, P, lane);
            for (long long i = lane; i < min((long long)m, seg); i += 64) keys_out[seg0 + i] = buf[i];
        }
        hits += m;
    }
    if (lane == 0) {
        if (!EMIT) count[row] = hits;
        else if (hits != seg) atomicAdd(&flags[RR_FLAG_MISMATCH], 1ull);
    }
}

// the heavy queries' segments, as the segmented sort takes them
__global__ __launch_bounds__(256) void sp_radius_segments_kernel(long long nheavy, long long q0,
                                                                 const int *__restrict__ heavy,
                                                                 const long long *__restrict__ off,
                                                                 long long *__restrict__ seg_lo,
                                                                 long long *__restrict__ seg_hi) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nheavy) return;
    const long long row = (long long)heavy[i] - q0;
    seg_lo[i] = off[row];
    seg_hi[i] = off[row + 1];
}

// ---- host side ----------------------------------------------------------------------------------------------------
// Both passes of a radius call over the queries [q0, q0 + nq) of the query side (the caller has reset the search's
// counters and counted the zero queries where they come from the index): R1, the scan, indptr_out, the cap, R2, the
// sort of the heavy segments, R3; the trace.  `who` names the entry point in messages.
template <int METRIC>
static int sp_radius_passes(fdr_ctx *ctx, const char *who, const SpQuerySide &qs, float radius, int64_t q0, int64_t nq,
                            int64_t max_hits, int64_t *indptr_out) {
    int rc;
    const hipStream_t st = ctx->stream;
    SparseIndex &sp = ctx->sp;
    SparseRadius &sr = ctx->spr;
    RadiusResult &rr = sr.rr;
    const RadiusCall call = {st, who, nq, max_hits, indptr_out};
    constexpr bool JAC = METRIC == FDR_METRIC_JACCARD;
    constexpr bool WJ = METRIC == FDR_METRIC_WEIGHTED_JACCARD;
    const int64_t n = sp.built.n;
    const long long nzero = sp.built.nzero;
    if ((rc = radius_reserve(rr, call))) return rc;
    if ((rc = sr.handed.reserve((size_t)nq))) return rc;
    HIP_TRY(hipMemsetAsync(sr.handed.ptr(), 0, (size_t)nq, st));
    auto launch = [&](auto range, auto emit, unsigned grid, u64 *keys_out) {  // (keys_out: R2's)
        hipLaunchKernelGGL((sp_radius_kernel<decltype(range)::value, decltype(emit)::value, METRIC>), dim3(grid), dim3(64),
                           0, st, (long long)n, (long long)q0, qs, sp.runptr.ptr(), sp.posting_rows(),
                           JAC ? nullptr : sp.pval.ptr(), JAC ? sp.asize.ptr() : nullptr, WJ ? sp.mass.ptr() : nullptr,
                           radius, nzero, rr.zlist.ptr(), sp.cnt.ptr(), rr.count.ptr(), sr.handed.ptr(), rr.off.ptr(),
                           keys_out, rr.flags.ptr());
    };
    // R1
    launch(std::false_type{}, std::false_type{}, (unsigned)nq, nullptr);
    HIP_TRY(hipGetLastError());
    u64 h[2] = {0, 0};  // queries for the range form; zero (empty) rows among the queries
    static_assert(SP_CNT_ZEROQ == SP_CNT_HEAVY + 1, "one read-back for both");
    HIP_TRY(hipMemcpyAsync(h, sp.cnt.ptr() + SP_CNT_HEAVY, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h[0] > (u64)nq)
        return fail(FDR_E_HIP, "internal: %s: %llu heavy queries of %lld", who, (unsigned long long)h[0], (long long)nq);
    if (h[0] > 0) {
        launch(std::true_type{}, std::false_type{}, (unsigned)h[0], nullptr);
        HIP_TRY(hipGetLastError());
    }
    fdr_knn_trace &t = ctx->last.trace;
    t.kind = FDR_TRACE_SPARSE;
    t.k = 0;
    t.queries = nq;
    t.targets = n;
    t.zero_queries = (int32_t)std::min<u64>(h[1], INT32_MAX);
    t.range_queries = (int32_t)h[0];
    t.range_chunks = h[0] ? (int32_t)((n + SP_W - 1) / SP_W) : 0;
    if ((rc = radius_offsets(rr, sp.tmp, call, "hits", "counts", nullptr)) || rr.counted == 0) return rc;
    const long long total = rr.counted;
    // R2
    const bool zeros = h[1] > 0 && nzero > 0;  // a zero query, and zero rows for it
    if (zeros && (rc = radius_zero_list(rr, sp.tmp, call, sp.zero.ptr(), n, nzero))) return rc;
    if (h[0] > 0) {
        if ((rc = sr.seg_lo.reserve((size_t)h[0]))) return rc;
        if ((rc = sr.seg_hi.reserve((size_t)h[0]))) return rc;
        hipLaunchKernelGGL(sp_radius_segments_kernel, dim3((unsigned)((h[0] + 255) / 256)), dim3(256), 0, st,
                           (long long)h[0], (long long)q0, qs.heavy, rr.off.ptr(), sr.seg_lo.ptr(), sr.seg_hi.ptr());
        HIP_TRY(hipGetLastError());
        launch(std::true_type{}, std::true_type{}, (unsigned)h[0], rr.keys.ptr());
        HIP_TRY(hipGetLastError());
        auto sort = [&](void *tmp, size_t &bytes) {  // (dist <= r < 1: the keys lie below 2^62)
            return rocprim::segmented_radix_sort_keys(tmp, bytes, rr.keys.ptr(), rr.sorted.ptr(), (unsigned)total,
                                                      (unsigned)h[0], sr.seg_lo.ptr(), sr.seg_hi.ptr(), 0, 62, st);
        };
        if ((rc = rocprim_run(sp.tmp, "rocprim::segmented_radix_sort_keys", sort))) return rc;
    }
    launch(std::false_type{}, std::true_type{}, (unsigned)nq, rr.sorted.ptr());  // (every other query, sorted in LDS)
    HIP_TRY(hipGetLastError());
    // R3
    hipLaunchKernelGGL(radius_split_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total,
                       rr.sorted.ptr(), rr.idx(), reinterpret_cast<float *>(rr.idx() + total), 0ll,
                       (const long long *)nullptr, (const long long *)nullptr);
    HIP_TRY(hipGetLastError());
    if ((rc = radius_check(rr, call, zeros, nzero))) return rc;
    rr.held = total;
    return FDR_OK;
}

static int sp_radius(fdr_ctx *ctx, const char *who, const SpQuerySide &qs, float radius, int64_t q0, int64_t nq,
                     int64_t max_hits, int64_t *indptr_out) {
    if (ctx->sp.built.metric == FDR_METRIC_JACCARD)
        return sp_radius_passes<FDR_METRIC_JACCARD>(ctx, who, qs, radius, q0, nq, max_hits, indptr_out);
    if (ctx->sp.built.metric == FDR_METRIC_WEIGHTED_JACCARD)
        return sp_radius_passes<FDR_METRIC_WEIGHTED_JACCARD>(ctx, who, qs, radius, q0, nq, max_hits, indptr_out);
    return sp_radius_passes<FDR_METRIC_COSINE>(ctx, who, qs, radius, q0, nq, max_hits, indptr_out);
}

// what the two radius entries do first: no held result; the index, the radius, the cap
static int sp_radius_args(fdr_ctx *ctx, const char *who, float radius, int64_t max_hits) {
    ctx->spr.rr.drop();
    return radius_args(ctx->sp.built.valid, who, "sparse", "fdr_sparse_index_search", radius, max_hits);
}

// a call without queries: the trace, an empty result
static int sp_radius_none(fdr_ctx *ctx, int64_t *indptr_out) {
    fdr_knn_trace &t = ctx->last.trace;
    t.kind = FDR_TRACE_SPARSE;
    t.k = 0;
    t.queries = 0;
    t.targets = ctx->sp.built.n;
    return radius_none(ctx->spr.rr, indptr_out);
}

FDR_EXPORT int fdr_sparse_index_radius_search(fdr_ctx *ctx, float radius, int64_t q_lo, int64_t q_hi, int64_t max_hits,
                                              int64_t *indptr_out) {
    static const char who[] = "sparse_index_radius_search";
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    if ((rc = sp_radius_args(ctx, who, radius, max_hits))) return rc;
    SparseIndex &sp = ctx->sp;
    const int64_t n = sp.built.n;
    if (q_lo < 0 || q_hi < q_lo || q_hi > n)
        return fail(FDR_E_ARG, "%s: rows [%lld, %lld) are no range of the %lld rows", who, (long long)q_lo,
                    (long long)q_hi, (long long)n);
    if (!indptr_out) return fail(FDR_E_ARG, "%s: null pointer", who);
    const int64_t nq = q_hi - q_lo;
    if (nq == 0) return sp_radius_none(ctx, indptr_out);
    const hipStream_t st = ctx->stream;
    HIP_TRY(hipMemsetAsync(sp.cnt.ptr() + SP_CNT_HEAVY, 0, 16, st));  // (the heavy list's counter and the zero queries')
    if (sp.built.nzero > 0) {
        hipLaunchKernelGGL(sp_count_zero_kernel, dim3((unsigned)((nq + 4095) / 4096)), dim3(256), 0, st, (long long)q_lo,
                           (long long)q_hi, sp.zero.ptr(), sp.cnt.ptr());
        HIP_TRY(hipGetLastError());
    }
    const SpQuerySide own = {sp.indptr.ptr(), sp.efeat.ptr(), sp.xhat.ptr(),  sp.asize.ptr(),
                             sp.mass.ptr(),   sp.zero.ptr(),  sp.heavy.ptr()};
    return sp_radius(ctx, who, own, radius, q_lo, nq, max_hits, indptr_out);
}

FDR_EXPORT int fdr_sparse_index_radius_query(fdr_ctx *ctx, float radius, int64_t nq, const int64_t *q_indptr,
                                             const int32_t *q_indices, const float *q_values, int64_t max_hits,
                                             int64_t *indptr_out) {
    static const char who[] = "sparse_index_radius_query";
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    if ((rc = sp_radius_args(ctx, who, radius, max_hits))) return rc;
    if (nq < 0 || nq > INT32_MAX) return fail(FDR_E_ARG, "%s: nq (%lld) must be in [0, 2^31)", who, (long long)nq);
    if (!indptr_out) return fail(FDR_E_ARG, "%s: null pointer", who);
    if (nq == 0) return sp_radius_none(ctx, indptr_out);
    if (!q_indptr) return fail(FDR_E_ARG, "%s: null pointer", who);
    SpQuerySide side = {};
    u64 zeroq = 0;
    if ((rc = sp_query_side(ctx, who, nq, q_indptr, q_indices, q_values, side, zeroq))) return rc;
    return sp_radius(ctx, who, side, radius, 0, nq, max_hits, indptr_out);
}

FDR_EXPORT int fdr_sparse_index_radius_fetch(fdr_ctx *ctx, int64_t hits, int32_t *idx_out, float *dist_out) {
    if (int rc = use_device(ctx)) return rc;
    return radius_fetch(ctx->stream, ctx->spr.rr, "sparse_index_radius_fetch", "next sparse call", hits, idx_out, dist_out);
}
