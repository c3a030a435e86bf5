// Part of libfedrann_hip.so (included by fedrann_hip.hip, behind knn_radius_common.inc and topk_merge.inc).
//
// fdr_graph_symmetrize: one neighbour graph turned into another.  The input is a square graph on n rows as ragged rows
// (row q's entries (t, d): "q lists t at distance bits b(q->t)"), unsorted; the result's row r holds s
//     union      iff r lists s or s lists r, at the smaller bits of the directions present,
//     mutual     iff r lists s and s lists r, at min(b(r->s), b(s->r)),
//     transpose  iff s lists r, at b(s->r),
// each row strictly ascending by key = bits << 32 | index.  fedrann_amd.graph.symmetrize_rows is the model of this file,
// bit for bit, and the route without a GPU.  The protocol is the radius searches' (knn_radius_common.inc) on a
// RadiusResult of the call's own: count, scan, indptr_out, the cap, emit into the counted segments, sort, split,
// cross-check, hold.  The refusal record is topk_merge.inc's idea: the smallest (row << 8 | rule) by one atomicMin per
// wave that saw a violation.
//
// G1  gs_pack_kernel, one thread per entry: the entry's row (a binary search in the indptr, kept for G2 and G3: the
//     segmented sort leaves every entry in its row's segment), the index and distance rules, the key index << 32 | bits.
//     rocprim::segmented_radix_sort_keys over the input rows then gives every row ordered by index.
// G2  gs_count_kernel, one thread per entry (q -> t) of that copy.  The repeated-index rule is one comparison with the
//     entry before it in the row.  A binary search of row t's entries for q says whether t lists q and at which bits
//     (the two directions need not agree); the answer is kept per entry (4 bytes) so that G3 does not search again.
//     Counts: union count[q] += 1 and count[t] += 1 without a partner; mutual count[q] += partner; transpose
//     count[t] += 1.  A self entry finds itself.  The adds to count[q] are one atomic per (wave, row): the lanes of a
//     row are neighbours in the wave (gs_row_add).  Those to count[t] are one atomic each: a row's t are distinct, so
//     lanes share a destination only across rows; a hub listed by 20 000 rows costs 20 000 threads' single adds.
//     Integer atomics: the totals do not depend on the order of arrival.
// G3  gs_emit_kernel, the same walk: bits << 32 | index into the counted segment.  Union puts row q's own entries at
//     the head of its segment by position and the reverse entries behind them through the row's cursor; mutual and
//     transpose place through the cursor alone.  The arrival order is forgotten by G4.
// G4  segmented sort of the result rows by key (an index appears once per row: the keys of a row are distinct, so the
//     sorted row is a function of the input alone), radius_split_kernel<false>, and gs_check_kernel: every row's
//     cursor stands where the count said it would, or the call fails as an internal error.
//
// Device bytes held: 32 per input entry (index 4, distance 4, row 4, packed key 8, ordered key 8, partner bits 4), 16 per
// result entry (the keys as emitted and as sorted; the held indices and distances take the former's place), 28 per row
// (the input's indptr, the counts, their scan, the cursor).
// Bounds: the host has checked the indptr (it starts at 0, never decreases, totals below 2^31) before the upload, so a
// row's segment lies in [0, total); G2 searches row t only for 0 <= t < n whatever the entry holds, and G3 runs only
// after the host has read an empty refusal record; every store of G3 is checked against the end of its row's segment.
// The front (the host's indptr check, the upload, G1 and the sort by index: gs_check_indptr, gs_rows_by_index), the
// reverse search of G2 (gs_reverse_bits) and the refusal's words (gs_refused) are functions, because
// fdr_graph_components (graph_components.inc) starts from the same rows.

constexpr unsigned GS_NO_PARTNER = 0xffffffffu;  // (a listed distance's bits are at most 0x7f800000)
enum { GS_RULE_INDEX = 1, GS_RULE_DISTANCE = 2, GS_RULE_REPEAT = 3 };

// every lane of the wave calls: the smallest record of the wave, where there is one, in one atomicMin
__device__ __forceinline__ void gs_refuse(u64 bad, u64 *__restrict__ refusal) {
    if (__ballot(bad != TM_NONE)) {
        bad = tm_wave_min(bad, 64);
        if ((threadIdx.x & 63) == 0) atomicMin(refusal, bad);
    }
}

// Every lane of the wave calls.  The live lanes hold entries of rows q that never decrease along the wave, so the
// lanes of one row are neighbours.  One atomicAdd per row of the wave adds the row's flagged lanes to counter[q]; a
// flagged lane gets what the add returned plus the flagged lanes of its row below it (its own slot behind the cursor).
template <class T>
__device__ __forceinline__ T gs_row_add(int lane, bool live, int q, bool flag, T *__restrict__ counter) {
    const int prev = __shfl_up(q, 1, 64);
    const bool head = !live || lane == 0 || prev != q;  // (a lane without an entry is a run of its own)
    const u64 heads = __ballot(head), flags = __ballot(live && flag);
    const int first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));  // the last head at or below this lane
    const u64 above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    const int end = above ? __ffsll((long long)above) - 1 : 64;  // the next head above it
    const u64 run = (end == 64 ? ~0ull : (1ull << end) - 1) & (~0ull << first);
    const int mine = __popcll(flags & run);
    T base = 0;
    if (lane == first && live && mine) base = atomicAdd(&counter[q], (T)mine);
    base = __shfl(base, first, 64);
    return base + (T)__popcll(flags & run & ((1ull << lane) - 1));
}

__global__ __launch_bounds__(256) void gs_pack_kernel(long long total, long long n, const long long *__restrict__ indptr,
                                                      const int *__restrict__ idx, const float *__restrict__ dist,
                                                      int *__restrict__ row, u64 *__restrict__ packed,
                                                      u64 *__restrict__ refusal) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    u64 bad = TM_NONE;
    if (i < total) {
        long long lo = 0, hi = n;  // the r in [0, n) with indptr[r] <= i < indptr[r + 1]  (indptr[0] = 0, indptr[n] = total)
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (indptr[mid] <= i) lo = mid;
            else hi = mid;
        }
        const int t = idx[i];
        const unsigned bits = __float_as_uint(dist[i]);
        row[i] = (int)lo;
        packed[i] = ((u64)(unsigned)t << 32) | bits;
        int rule = 0;
        if (t < 0 || (long long)t >= n) rule = GS_RULE_INDEX;
        else if (bits > 0x7f800000u) rule = GS_RULE_DISTANCE;
        if (rule) bad = ((u64)lo << 8) | (u64)rule;
    }
    gs_refuse(bad, refusal);
}

// The reverse of an entry (q -> t), 0 <= t < n, among the rows ordered by index: a binary search of row t's entries for
// q.  The bits of (t -> q), or GS_NO_PARTNER where t does not list q.  (graph_components.inc searches with it too.)
__device__ __forceinline__ unsigned gs_reverse_bits(const long long *__restrict__ indptr, const u64 *__restrict__ byidx,
                                                    long long t, int q) {
    const long long end = indptr[t + 1];
    long long lo = indptr[t], hi = end;  // the first entry of row t with index >= q
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((unsigned)(byidx[mid] >> 32) < (unsigned)q) lo = mid + 1;
        else hi = mid;
    }
    if (lo < end) {
        const u64 found = byidx[lo];
        if ((unsigned)(found >> 32) == (unsigned)q) return (unsigned)found;
    }
    return GS_NO_PARTNER;
}

template <int MODE>
__global__ __launch_bounds__(256) void gs_count_kernel(long long total, long long n, const long long *__restrict__ indptr,
                                                       const int *__restrict__ row, const u64 *__restrict__ byidx,
                                                       unsigned *__restrict__ partner,
                                                       unsigned long long *__restrict__ count,
                                                       u64 *__restrict__ refusal) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < total;
    u64 bad = TM_NONE;
    int q = 0;
    long long t = -1;  // the listed row, where it is one
    bool has = false;
    if (live) {
        q = row[i];
        const unsigned listed = (unsigned)(byidx[i] >> 32);
        if (i > indptr[q] && (unsigned)(byidx[i - 1] >> 32) == listed) bad = ((u64)q << 8) | (u64)GS_RULE_REPEAT;
        unsigned pb = GS_NO_PARTNER;
        if ((long long)listed < n) {  // (G1 refuses every other entry; here the test keeps the search inside the rows)
            t = listed;
            pb = gs_reverse_bits(indptr, byidx, t, q);
        }
        partner[i] = pb;
        has = pb != GS_NO_PARTNER;
    }
    gs_refuse(bad, refusal);
    if (MODE != FDR_GRAPH_TRANSPOSE) gs_row_add(lane, live, q, MODE == FDR_GRAPH_UNION || has, count);
    if (t >= 0 && (MODE == FDR_GRAPH_TRANSPOSE || (MODE == FDR_GRAPH_UNION && !has))) atomicAdd(&count[t], 1ull);
}

template <int MODE>
__global__ __launch_bounds__(256) void gs_emit_kernel(long long total, long long n, const long long *__restrict__ indptr,
                                                      const int *__restrict__ row, const u64 *__restrict__ byidx,
                                                      const unsigned *__restrict__ partner,
                                                      const long long *__restrict__ off, unsigned *__restrict__ fill,
                                                      u64 *__restrict__ keys, u64 *__restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < total;
    int q = 0;
    long long t = -1;
    unsigned bits = 0, low = 0;
    bool has = false;
    if (live) {
        q = row[i];
        const u64 key = byidx[i];
        const unsigned pb = partner[i];
        bits = (unsigned)key;
        has = pb != GS_NO_PARTNER;
        low = has && pb < bits ? pb : bits;
        if ((long long)(key >> 32) < n) t = (long long)(key >> 32);
    }
    // (segment, position in it, key): stored inside the segment, or counted as a mismatch
    auto place = [&](long long r, long long at, u64 key) {
        const long long pos = off[r] + at;
        if (pos < off[r + 1]) keys[pos] = key;
        else atomicAdd(&flags[RR_FLAG_MISMATCH], 1ull);
    };
    if (MODE == FDR_GRAPH_UNION) {
        if (t >= 0) {
            place(q, i - indptr[q], ((u64)low << 32) | (u64)t);
            if (!has) place(t, indptr[t + 1] - indptr[t] + (long long)atomicAdd(&fill[t], 1u), ((u64)bits << 32) | (unsigned)q);
        }
    } else if (MODE == FDR_GRAPH_MUTUAL) {
        const unsigned at = gs_row_add(lane, live, q, has, fill);
        if (has && t >= 0) place(q, at, ((u64)low << 32) | (u64)t);
    } else {
        if (t >= 0) place(t, atomicAdd(&fill[t], 1u), ((u64)bits << 32) | (unsigned)q);
    }
}

// every row's cursor against its count (union: less the row's own entries, which took no cursor)
template <int MODE>
__global__ __launch_bounds__(256) void gs_check_kernel(long long n, const long long *__restrict__ indptr,
                                                       const long long *__restrict__ count,
                                                       const unsigned *__restrict__ fill, u64 *__restrict__ flags) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    bool off = false;
    if (r < n) off = (long long)fill[r] != count[r] - (MODE == FDR_GRAPH_UNION ? indptr[r + 1] - indptr[r] : 0ll);
    const u64 m = __ballot(off);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&flags[RR_FLAG_MISMATCH], (u64)__popcll(m));
}

// G2, G3 and the check of `mode` over `total` input entries
static int gs_passes(int mode, int pass, hipStream_t st, GraphSymScratch &gs, long long total, long long n) {
    RadiusResult &rr = gs.rr;
    const dim3 grid((unsigned)((total + 255) / 256)), rows((unsigned)((n + 255) / 256)), block(256);
    auto run = [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        if (pass == 2)
            hipLaunchKernelGGL(gs_count_kernel<MODE>, grid, block, 0, st, total, n, gs.indptr.ptr(), gs.row.ptr(),
                               gs.byidx.ptr(), gs.partner.ptr(), reinterpret_cast<unsigned long long *>(rr.count.ptr()),
                               gs.refusal.ptr());
        else if (pass == 3)
            hipLaunchKernelGGL(gs_emit_kernel<MODE>, grid, block, 0, st, total, n, gs.indptr.ptr(), gs.row.ptr(),
                               gs.byidx.ptr(), gs.partner.ptr(), rr.off.ptr(), gs.fill.ptr(), rr.keys.ptr(),
                               rr.flags.ptr());
        else
            hipLaunchKernelGGL(gs_check_kernel<MODE>, rows, block, 0, st, n, gs.indptr.ptr(), rr.count.ptr(),
                               gs.fill.ptr(), rr.flags.ptr());
    };
    if (mode == FDR_GRAPH_UNION) run(std::integral_constant<int, FDR_GRAPH_UNION>{});
    else if (mode == FDR_GRAPH_MUTUAL) run(std::integral_constant<int, FDR_GRAPH_MUTUAL>{});
    else run(std::integral_constant<int, FDR_GRAPH_TRANSPOSE>{});
    HIP_TRY(hipGetLastError());
    return FDR_OK;
}

// ---- the front that fdr_graph_symmetrize and fdr_graph_components (graph_components.inc) share ----
// The indptr, on the host: what keeps the kernels' loads in bounds.
static int gs_check_indptr(const char *who, int64_t n, const int64_t *indptr) {
    if (indptr[0] != 0) return fail(FDR_E_ARG, "%s: the indptr starts at %lld, not 0", who, (long long)indptr[0]);
    for (int64_t r = 0; r < n; ++r)
        if (indptr[r + 1] < indptr[r]) return fail(FDR_E_ARG, "%s: row %lld: the indptr decreases", who, (long long)r);
    if (indptr[n] > INT32_MAX) return fail(FDR_E_ARG, "%s: the graph holds 2^31 entries or more", who);
    return FDR_OK;
}

// The graph (a checked indptr, total = indptr[n] > 0 entries) to the device, an empty refusal record, G1, and every row
// ordered by index in gs.byidx.  Enqueues only.
static int gs_rows_by_index(hipStream_t st, GraphSymScratch &gs, int64_t n, long long total, const int64_t *indptr,
                            const int32_t *idx, const float *dist) {
    int rc;
    const size_t rows = (size_t)n + 1;
    if ((rc = gs.indptr.reserve(rows))) return rc;
    if ((rc = gs.idx.reserve((size_t)total))) return rc;
    if ((rc = gs.dist.reserve((size_t)total))) return rc;
    if ((rc = gs.row.reserve((size_t)total))) return rc;
    if ((rc = gs.packed.reserve((size_t)total))) return rc;
    if ((rc = gs.byidx.reserve((size_t)total))) return rc;
    if ((rc = gs.refusal.reserve(1))) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "the caller's indptr is the device's");
    HIP_TRY(upload(gs.indptr, reinterpret_cast<const long long *>(indptr), rows, st));
    HIP_TRY(upload(gs.idx, idx, (size_t)total, st));
    HIP_TRY(upload(gs.dist, dist, (size_t)total, st));
    HIP_TRY(hipMemsetAsync(gs.refusal.ptr(), 0xff, 8, st));
    // G1, and the rows by index
    hipLaunchKernelGGL(gs_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, (long long)n,
                       gs.indptr.ptr(), gs.idx.ptr(), gs.dist.ptr(), gs.row.ptr(), gs.packed.ptr(), gs.refusal.ptr());
    HIP_TRY(hipGetLastError());
    // (All 64 bits, not [32, 64): the order by (index, bits) serves as well, and rocprim's comparator for short segments
    // builds its mask with a shift by begin_bit + length, which a range that ends at bit 64 but starts above 0 overflows.)
    auto by_index = [&](void *tmp, size_t &bytes) {
        return rocprim::segmented_radix_sort_keys(tmp, bytes, gs.packed.ptr(), gs.byidx.ptr(), (unsigned)total, (unsigned)n,
                                                  gs.indptr.ptr(), gs.indptr.ptr() + 1, 0, 64, st);
    };
    return rocprim_run(gs.tmp, "rocprim::segmented_radix_sort_keys", by_index);
}

// a refusal record that the host has read and found set: the call's error
static int gs_refused(const char *who, u64 refused) {
    const int rule = (int)(refused & 0xff);
    const char *what = rule == GS_RULE_INDEX      ? "an index outside [0, n)"
                       : rule == GS_RULE_DISTANCE ? "a distance that is negative or NaN (its bits must be at most 0x7f800000)"
                                                  : "an index listed twice";
    return fail(FDR_E_ARG, "%s: row %lld: %s", who, (long long)(refused >> 8), what);
}

FDR_EXPORT int fdr_graph_symmetrize(fdr_ctx *ctx, int32_t mode, int64_t n, const int64_t *indptr, const int32_t *idx,
                                    const float *dist, int64_t max_entries, int64_t *indptr_out) {
    static const char who[] = "graph_symmetrize";
    int rc = use_device(ctx);
    if (rc) return rc;
    GraphSymScratch &gs = ctx->gs;
    RadiusResult &rr = gs.rr;
    rr.drop();
    if (mode != FDR_GRAPH_UNION && mode != FDR_GRAPH_MUTUAL && mode != FDR_GRAPH_TRANSPOSE)
        return fail(FDR_E_ARG, "%s: mode %d is none of FDR_GRAPH_UNION, _MUTUAL, _TRANSPOSE", who, mode);
    if (n < 1 || n > INT32_MAX) return fail(FDR_E_ARG, "%s: n (%lld) must be in [1, 2^31)", who, (long long)n);
    if (max_entries < 1 || max_entries > INT32_MAX)
        return fail(FDR_E_ARG, "%s: max_entries (%lld) must be in [1, 2^31)", who, (long long)max_entries);
    if (!indptr || !indptr_out) return fail(FDR_E_ARG, "%s: null indptr pointer", who);
    if ((rc = gs_check_indptr(who, n, indptr))) return rc;
    const long long total = indptr[n];
    const size_t rows = (size_t)n + 1;
    if (total == 0) {  // (no entries: an empty result, held)
        for (size_t r = 0; r < rows; ++r) indptr_out[r] = 0;
        rr.counted = 0;
        rr.held = 0;
        return FDR_OK;
    }
    if (!idx || !dist) return fail(FDR_E_ARG, "%s: null pointer", who);
    const hipStream_t st = ctx->stream;
    const RadiusCall call = {st, who, n, max_entries, indptr_out};
    if ((rc = radius_reserve(rr, call))) return rc;
    if ((rc = gs.partner.reserve((size_t)total))) return rc;
    if ((rc = gs.fill.reserve((size_t)n))) return rc;
    HIP_TRY(hipMemsetAsync(gs.fill.ptr(), 0, (size_t)n * 4, st));
    const dim3 block(256);
    // G1, and the rows by index
    if ((rc = gs_rows_by_index(st, gs, n, total, indptr, idx, dist))) return rc;
    // G2, the scan, the refusal record, indptr_out, the cap
    if ((rc = gs_passes(mode, 2, st, gs, total, n))) return rc;
    if ((rc = radius_scan(rr, gs.tmp, call, rr.off.ptr()))) return rc;
    gs.h_off.resize(rows);
    u64 refused = TM_NONE;
    HIP_TRY(download(gs.h_off.data(), rr.off, rows, st));
    HIP_TRY(download(&refused, gs.refusal, 1, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (refused != TM_NONE) return gs_refused(who, refused);  // (nothing has been written to indptr_out)
    for (size_t r = 0; r < rows; ++r) indptr_out[r] = gs.h_off[r];
    const long long out = rr.counted = gs.h_off[n];
    if (out > max_entries)  // (the one refusal that has written its output, as the radius searches')
        return fail(FDR_E_ARG, "%s: %lld entries exceed max_entries = %lld (indptr_out holds the counts)", who, out,
                    (long long)max_entries);
    if (out == 0) {  // (mutual rows of a graph without a reciprocated pair)
        rr.held = 0;
        return FDR_OK;
    }
    if ((rc = rr.keys.reserve((size_t)out))) return rc;
    if ((rc = rr.sorted.reserve((size_t)out))) return rc;
    // G3, G4
    if ((rc = gs_passes(mode, 3, st, gs, total, n))) return rc;
    auto by_key = [&](void *tmp, size_t &bytes) {  // (bits <= 0x7f800000: the keys lie below 2^63)
        return rocprim::segmented_radix_sort_keys(tmp, bytes, rr.keys.ptr(), rr.sorted.ptr(), (unsigned)out, (unsigned)n,
                                                  rr.off.ptr(), rr.off.ptr() + 1, 0, 63, st);
    };
    if ((rc = rocprim_run(gs.tmp, "rocprim::segmented_radix_sort_keys", by_key))) return rc;
    hipLaunchKernelGGL(radius_split_kernel<false>, dim3((unsigned)((out + 255) / 256)), block, 0, st, out, rr.sorted.ptr(),
                       rr.idx(), reinterpret_cast<float *>(rr.idx() + out), 0ll, (const long long *)nullptr,
                       (const long long *)nullptr);
    HIP_TRY(hipGetLastError());
    if ((rc = gs_passes(mode, 4, st, gs, total, n))) return rc;
    u64 f[RR_FLAGS] = {};
    HIP_TRY(download(f, rr.flags, RR_FLAGS, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (f[RR_FLAG_MISMATCH] != 0)
        return fail(FDR_E_HIP, "internal: %s: the emit pass disagrees with the count pass on %llu rows or entries", who,
                    (unsigned long long)f[RR_FLAG_MISMATCH]);
    rr.held = out;
    return FDR_OK;
}

FDR_EXPORT int fdr_graph_symmetrize_fetch(fdr_ctx *ctx, int64_t entries, int32_t *idx_out, float *dist_out) {
    static const char who[] = "graph_symmetrize_fetch";
    if (int rc = use_device(ctx)) return rc;
    const RadiusResult &rr = ctx->gs.rr;
    if (rr.held < 0)  // (radius_fetch's two refusals, in this call's words)
        return fail(FDR_E_STATE, "%s: the context holds no symmetrised graph (the next fdr_graph_symmetrize and "
                    "fdr_graph_free drop it)", who);
    if (entries != rr.held)
        return fail(FDR_E_ARG, "%s: entries = %lld, the held result has %lld", who, (long long)entries, rr.held);
    return radius_fetch(ctx->stream, ctx->gs.rr, who, "next fdr_graph_symmetrize", entries, idx_out, dist_out);
}

FDR_EXPORT int fdr_graph_free(fdr_ctx *ctx) {
    if (int rc = use_device(ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->gs.release();
    ctx->gc.release();
    ctx->ge.release();
    return FDR_OK;
}
