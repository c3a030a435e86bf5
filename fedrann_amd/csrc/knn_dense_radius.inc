// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit) behind knn_sparse_radius.inc.
// ------------------------------------------------------------------------------------------
// D-R1 .. D-R3  radius search on the dense index (fdr_dense_index_radius_search / _query / _fetch): every index row
// within a cosine distance bound r of each query, 0 <= r < 1, on the projected (embedded) rows.
//
// The index (DenseIndex, fedrann_hip.hip) holds the normalised rows (fdr_normalize_dev's layout), their fp16 copy and
// the zero-row flags.  The fp16 range pass (knn_range_kernel / knn_range_pp_kernel, the shape range_shape() picks for
// the call's queries) finds, per query, every target with approximate distance d~ <= th, th = r + radius_margin()
// (knn_plan.inc: a superset of the rows with canonical distance <= r), and the canonical fp32 chain decides.  The
// protocol around the passes (the scan, the cap, the zero rows' list, the cross-check, the held result) is
// knn_radius_common.inc's; what it counts and caps here are the CANDIDATES, upper bounds of the hit counts.
//   D-R1  the range pass with the RangeCount sink: each lane counts its query's candidates in a register and adds
//         them to count[q] with one atomic at the end.  A zero query takes no part (its threshold is -inf): its count
//         is the index's zero rows.
//   D-R2  the same pass with the RangeEmit sink: a lane's candidates wait in its LDS buffer, as RangeHits' do, and
//         leave with one returning atomic per batch into the query's segment, bounded by what D-R1 counted.
//   D-R3  dr_exact_kernel, one wave per query: the canonical chain (canonical_chain, knn_rerank_long_kernel's own)
//         over the segment, key = dist_bits << 32 | row where dist <= r, else KEY_INF; the hits are counted.  Then
//         the scan of the hit counts (the exact indptr), ONE rocprim segmented radix sort over the candidate segments
//         (the misses sort to each segment's tail) and radius_split_kernel<true>, the compacting form: the first
//         count[q] keys of each segment -> idx / dist.
// Memory: 16 bytes per candidate (8 of keys, which take the result afterwards; 8 of sorted keys, whose first half
// holds D-R2's rows before the sort), 32 bytes per query of the largest call, 4 per zero row.
// Cost model: two fp16 scans of queries x targets at the staging rate plus a tail proportional to the candidates
// (one row read and one chain each, the sort): DESIGN.md section 5.
// An index of more than 96 << 19 rows, what one plan of the fp16 shapes holds, is scanned in target chunks (dr_scan).
// Out of scope: duplicate-row classes, live-chunk skipping, several devices, d > 512.
// ------------------------------------------------------------------------------------------

// ---- the sinks of the range kernels (RangeHits, knn_prefilter.inc, is the k-NN search's) ----------------------------
struct RangeCountOut {
    unsigned long long *count;  // [nq] candidates per query
};
template <int NT>
struct RangeCount {
    typedef RangeCountOut Out;
    unsigned long long *count;
    int qg, lcount;
    static __device__ __forceinline__ RangeCount make(int *, const Out &o, int qg, int) { return RangeCount{o.count, qg, 0}; }
    __device__ __forceinline__ void add(int) { ++lcount; }
    __device__ __forceinline__ void finish() {
        if (lcount > 0) atomicAdd(count + qg, (unsigned long long)lcount);
    }
};

struct RangeEmitOut {
    int *fill;             // [nq] rows emitted so far (may pass the segment's length: the excess is not written)
    const long long *off;  // [nq + 1] the segments D-R1 counted
    int *rows;             // [off[nq]] the candidates' target rows
};
template <int NT>
struct RangeEmit {
    typedef RangeEmitOut Out;
    int *lbuf;  // [RANGE_LANE_BUF][NT], as RangeHits'
    Out out;
    int qg, tid, lcount;
    static __device__ __forceinline__ RangeEmit make(int *lbuf, const Out &o, int qg, int tid) {
        return RangeEmit{lbuf, o, qg, tid, 0};
    }
    __device__ __forceinline__ void flush() {
        const long long pos = atomicAdd(out.fill + qg, lcount);
        const long long seg0 = out.off[qg], seg = out.off[qg + 1] - seg0;  // (read on the rare path only: no registers held)
        for (int i = 0; i < lcount; ++i)
            if (pos + i < seg) out.rows[seg0 + pos + i] = lbuf[i * NT + tid];
        lcount = 0;
    }
    __device__ __forceinline__ void add(int row) {
        lbuf[lcount * NT + tid] = row;
        if (++lcount == RANGE_LANE_BUF) flush();
    }
    __device__ __forceinline__ void finish() {
        if (lcount > 0) flush();
    }
};

// the range kernel of kShapes[S] with another sink
template <int S, template <int> class SinkT>
static constexpr auto dr_range_kernel() {
    constexpr KnnShape e = kShapes[S];
    using Sink = SinkT<64 * e.nw>;
    using K = void (*)(const _Float16 *, const float *, int, const _Float16 *, int, int, SegBounds, typename Sink::Out);
    if constexpr (!shape_compiled<S>()) return (K) nullptr;
    else if constexpr (e.family == FDR_FAM_RANGE) return (K)knn_range_kernel<e.dp, e.nw, e.dp == 128 ? e.wps : 2, Sink>;
    else if constexpr (e.family == FDR_FAM_RANGE_PP) return (K)knn_range_pp_kernel<e.dp, e.units(), Sink>;
    else return (K) nullptr;
}
// (the shapes range_shape() gives a radius call: four waves below 4096 queries, the ping-pong skeleton from there)
template <template <int> class SinkT>
static auto dr_kernel_of(int shape) -> decltype(dr_range_kernel<FDR_R128, SinkT>()) {
    switch (shape) {
    case FDR_R128: return dr_range_kernel<FDR_R128, SinkT>();
    case FDR_R256: return dr_range_kernel<FDR_R256, SinkT>();
    case FDR_R512: return dr_range_kernel<FDR_R512, SinkT>();
    case FDR_RPP128: return dr_range_kernel<FDR_RPP128, SinkT>();
    case FDR_RPP256: return dr_range_kernel<FDR_RPP256, SinkT>();
    case FDR_RPP512: return dr_range_kernel<FDR_RPP512, SinkT>();
    default: return nullptr;
    }
}

// ---- small kernels ---------------------------------------------------------------------------------------------------
// per query: its threshold (a zero query: -inf, no candidate) and, for a zero query, its count, the index's zero rows
__global__ __launch_bounds__(256) void dr_prepare_kernel(long long nq, const unsigned char *__restrict__ qzero, float th,
                                                         long long nzero, float *__restrict__ theta,
                                                         long long *__restrict__ count, u64 *__restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool z = i < nq && qzero[i] != 0;
    if (i < nq) {
        theta[i] = z ? -__builtin_inff() : th;
        if (z) count[i] = nzero;
    }
    const u64 m = __ballot(z);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&flags[RR_FLAG_ZEROQ], (u64)__popcll(m));
}

// D-R3: one wave per query.  rows / keys [off[nq]]: the query's segment is [off[q], off[q + 1]); fill [nq]: what D-R2
// emitted; count [nq]: out, the hits.
__global__ __launch_bounds__(256) void dr_exact_kernel(long long nq, long long n, int DP, const float *__restrict__ Qhat,
                                                       const unsigned char *__restrict__ qzero,
                                                       const float *__restrict__ That, float radius,
                                                       const long long *__restrict__ off, const int *__restrict__ rows,
                                                       const int *__restrict__ fill, long long nzero,
                                                       const int *__restrict__ zlist, u64 *__restrict__ keys,
                                                       long long *__restrict__ count, u64 *__restrict__ flags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * 4 + wave;
    if (q >= nq) return;
    const long long seg0 = off[q], seg = off[q + 1] - seg0;
    if (qzero[q]) {  // every zero row of the index, at distance 0 (radius_emit_zero, written out: see there)
        for (long long m = lane; m < min(seg, nzero); m += 64) keys[seg0 + m] = (u64)(unsigned)zlist[m];
        if (lane == 0) {
            count[q] = min(seg, nzero);
            if (seg != nzero) atomicAdd(&flags[RR_FLAG_MISMATCH], 1ull);
        }
        return;
    }
    const long long got = fill[q];
    bool bad = got != seg;
    const f32x4 *qp = reinterpret_cast<const f32x4 *>(Qhat + (size_t)q * DP);
    int hits = 0;
    for (long long m = lane; m < seg; m += 64) {
        u64 key = KEY_INF;
        if (m < got) {
            const int t = rows[seg0 + m];
            if (t < 0 || (long long)t >= n) {
                bad = true;
            } else {
                const float c = canonical_chain(qp, reinterpret_cast<const f32x4 *>(That + (size_t)t * DP), DP);
                const float d = dist_from_sim(c);
                if (d <= radius) {
                    key = ((u64)__float_as_uint(d) << 32) | (unsigned)t;
                    ++hits;
                }
            }
        }
        keys[seg0 + m] = key;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) hits += __shfl_xor(hits, o);
    const bool anybad = __any(bad);
    if (lane == 0) {
        count[q] = hits;
        if (anybad) atomicAdd(&flags[RR_FLAG_MISMATCH], 1ull);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// One range scan of the call's queries over the whole index with the sink SinkT: a launch per target chunk
// (radius_chunks, knn_plan.inc: one below 50 331 648 rows), each with its own plan and its first row as t_base.  The
// sinks add to the same per-query counters from every chunk.  *nqb_out / *nseg_out: the query blocks, and the
// segments of all chunks together.
template <template <int> class SinkT, class Out>
static int dr_scan(fdr_ctx *ctx, const _Float16 *Qh, int64_t nq, int shape, const Out &out, int *nqb_out, int *nseg_out) {
    DenseIndex &di = ctx->di;
    const hipStream_t st = ctx->stream;
    const auto kern = dr_kernel_of<SinkT>(shape);
    if (!kern) return no_kernel(shape);
    const KnnShape &rsh = kShapes[shape];
    const size_t rlds = knn_lds_bytes(rsh, 1) + (size_t)RANGE_LANE_BUF * 64 * rsh.nw * 4;  // ring + lane buffers
    if (rsh.family == FDR_FAM_RANGE_PP)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rlds));
    int trc = timing_begin(ctx, FDR_KERNEL_KNN_PREFILTER, st);
    if (trc) return trc;
    const int64_t chunk = radius_chunk_rows(di.n);
    *nseg_out = 0;
    for (int64_t t0 = 0; t0 < di.n; t0 += chunk) {
        const int64_t rows = std::min<int64_t>(chunk, di.n - t0);
        const KnnPlan rp = knn_plan(ctx->num_cus, nq, rows, di.d, 1, shape);  // (k = 1: ring-only LDS, as the k-NN range pass)
        if (rp.nseg > FDR_MAX_SEG || rp.segs.b[rp.nseg] < rows)
            return fail(FDR_E_HIP, "internal: the range plan of %lld target rows has %d segments up to row %d",
                        (long long)rows, rp.nseg, rp.segs.b[std::min(rp.nseg, FDR_MAX_SEG)]);
        hipLaunchKernelGGL(kern, dim3((unsigned)rp.nqb, (unsigned)rp.nseg), dim3(64 * rsh.nw), rlds, st, Qh,
                           (const float *)di.theta.ptr(), (int)nq, (const _Float16 *)di.half.ptr() + (size_t)t0 * di.dp,
                           (int)rows, (int)t0, rp.segs, out);
        HIP_TRY(hipGetLastError());
        *nqb_out = rp.nqb;
        *nseg_out += rp.nseg;
    }
    return timing_end(ctx, FDR_KERNEL_KNN_PREFILTER, st);
}

// The passes of a radius call over nq queries: their normalised rows Qhat, fp16 copy Qh and zero flags on the device.
static int dr_radius_passes(fdr_ctx *ctx, const char *who, const float *Qhat, const _Float16 *Qh,
                            const unsigned char *qzero, float radius, int64_t nq, int64_t max_hits, int64_t *indptr_out) {
    int rc;
    const hipStream_t st = ctx->stream;
    DenseIndex &di = ctx->di;
    RadiusResult &rr = di.rr;
    const RadiusCall call = {st, who, nq, max_hits, indptr_out};
    const int64_t n = di.n;
    const long long nzero = di.nzero;
    di.last_candidates = di.last_hits = 0;
    if ((rc = radius_reserve(rr, call))) return rc;
    if ((rc = di.theta.reserve((size_t)nq))) return rc;
    if ((rc = di.ind.reserve((size_t)nq + 1))) return rc;
    if ((rc = di.fill.reserve((size_t)nq))) return rc;
    HIP_TRY(hipMemsetAsync(di.fill.ptr(), 0, (size_t)nq * 4, st));
    const float th = radius + radius_margin();
    hipLaunchKernelGGL(dr_prepare_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, (long long)nq, qzero, th,
                       nzero, di.theta.ptr(), rr.count.ptr(), rr.flags.ptr());
    HIP_TRY(hipGetLastError());
    int shape = range_shape(di.dp, (int)nq, (int)nq);
    if (shape == FDR_R128_W8) shape = FDR_R128;  // (a development knob's eight-wave form: not built with these sinks)
    // D-R1
    if ((rc = dr_scan<RangeCount>(ctx, Qh, nq, shape, RangeCountOut{reinterpret_cast<unsigned long long *>(rr.count.ptr())},
                                  &di.last_query_blocks, &di.last_segments)))
        return rc;
    u64 f[RR_FLAGS] = {};  // (with the offsets: the zero queries that dr_prepare_kernel counted)
    rc = radius_offsets(rr, di.tmp, call, "candidates", "candidate counts, upper bounds of the hit counts", f);
    const long long total = di.last_candidates = rr.counted;
    if (rc || total == 0) return rc;  // (no candidate, no hit: the counts are exact)
    // D-R2 (the rows wait in the first half of `sorted`, which the sort overwrites once D-R3 has read them)
    int *rows = reinterpret_cast<int *>(rr.sorted.ptr());
    const bool zeros = f[RR_FLAG_ZEROQ] > 0 && nzero > 0;  // a zero query, and zero rows for it
    if (zeros && (rc = radius_zero_list(rr, di.tmp, call, di.zero.ptr(), n, nzero))) return rc;
    if ((rc = dr_scan<RangeEmit>(ctx, Qh, nq, shape, RangeEmitOut{di.fill.ptr(), rr.off.ptr(), rows}, &di.last_query_blocks,
                                 &di.last_segments)))
        return rc;
    // D-R3
    if ((rc = timing_begin(ctx, FDR_KERNEL_KNN_RERANK, st))) return rc;
    hipLaunchKernelGGL(dr_exact_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, (long long)nq, (long long)n, di.dp,
                       Qhat, qzero, (const float *)di.ehat.ptr(), radius, (const long long *)rr.off.ptr(), (const int *)rows,
                       (const int *)di.fill.ptr(), nzero, (const int *)rr.zlist.ptr(), rr.keys.ptr(), rr.count.ptr(),
                       rr.flags.ptr());
    HIP_TRY(hipGetLastError());
    if ((rc = radius_scan(rr, di.tmp, call, di.ind.ptr()))) return rc;
    auto sort = [&](void *tmp, size_t &bytes) {  // (KEY_INF, a miss, lies below 2^63 and above every hit)
        return rocprim::segmented_radix_sort_keys(tmp, bytes, rr.keys.ptr(), rr.sorted.ptr(), (unsigned)total, (unsigned)nq,
                                                  rr.off.ptr(), rr.off.ptr() + 1, 0, 63, st);
    };
    if ((rc = rocprim_run(di.tmp, "rocprim::segmented_radix_sort_keys", sort))) return rc;
    HIP_TRY(hipMemcpyAsync(indptr_out, di.ind.ptr(), ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, st));
    if ((rc = radius_check(rr, call, zeros, nzero))) return rc;
    const int64_t hits = indptr_out[nq];
    if (hits < 0 || hits > total) return fail(FDR_E_HIP, "internal: %s: %lld hits of %lld candidates", who, (long long)hits, total);
    if (hits > 0) {
        hipLaunchKernelGGL(radius_split_kernel<true>, dim3((unsigned)((hits + 255) / 256)), dim3(256), 0, st, (long long)hits,
                           (const u64 *)rr.sorted.ptr(), rr.idx(), reinterpret_cast<float *>(rr.idx() + hits), (long long)nq,
                           (const long long *)di.ind.ptr(), (const long long *)rr.off.ptr());
        HIP_TRY(hipGetLastError());
    }
    if ((rc = timing_end(ctx, FDR_KERNEL_KNN_RERANK, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    di.last_hits = hits;
    rr.held = hits;
    return FDR_OK;
}

// E (device, [n, d], not normalised) -> the context's index
static int dr_index_from_device_E(fdr_ctx *ctx, const float *d_E, int64_t n, int d) {
    int rc;
    DenseIndex &di = ctx->di;
    const hipStream_t st = ctx->stream;
    const int dp = padded_dim(d);
    if ((rc = di.ehat.reserve((size_t)n * dp))) return rc;
    if ((rc = di.half.reserve((size_t)n * dp))) return rc;
    if ((rc = di.zero.reserve((size_t)n))) return rc;
    if ((rc = di.rr.flags.reserve(RR_FLAGS))) return rc;
    if ((rc = launch_normalize(ctx, d_E, n, d, di.ehat.ptr(), di.zero.ptr(), st))) return rc;
    hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)((n * (dp / 8) + 255) / 256)), dim3(256), 0, st,
                       (const float *)di.ehat.ptr(), (long long)n * (dp / 8), di.half.ptr());
    HIP_TRY(hipGetLastError());
    u64 *const d_nzero = di.rr.flags.ptr() + RR_FLAG_NZERO;
    HIP_TRY(hipMemsetAsync(di.rr.flags.ptr(), 0, RR_FLAGS * 8, st));
    hipLaunchKernelGGL(radius_count_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n,
                       (const unsigned char *)di.zero.ptr(), d_nzero);
    HIP_TRY(hipGetLastError());
    u64 nzero = 0;
    HIP_TRY(hipMemcpyAsync(&nzero, d_nzero, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    di.n = n;
    di.d = d;
    di.dp = dp;
    di.nzero = (long long)nzero;
    di.valid = true;
    return FDR_OK;
}

// what a build and an embed do first: no index, no held result, no figures of an earlier call
static void dr_index_reset(DenseIndex &di) {
    di.valid = false;
    di.rr.drop();
    di.last_candidates = di.last_hits = 0;
    di.last_query_blocks = di.last_segments = 0;
}

FDR_EXPORT int fdr_dense_index_build(fdr_ctx *ctx, const float *E, int64_t n, int32_t d) {
    int rc = use_device(ctx);
    if (rc) return rc;
    dr_index_reset(ctx->di);
    if (!E) return fail(FDR_E_ARG, "dense_index_build: null pointer");
    if (n < 1 || n > INT32_MAX) return fail(FDR_E_ARG, "dense_index_build: n (%lld) must be in [1, 2^31)", (long long)n);
    if (d < 1 || d > FDR_FAST_MAX_DIM)
        return fail(FDR_E_ARG, "dense_index_build: d = %d is outside [1, %d], the reach of the fp16 passes (the dense index "
                    "has no other path)", d, FDR_FAST_MAX_DIM);
    if ((rc = ctx->call.E.reserve((size_t)n * d))) return rc;
    HIP_TRY(upload(ctx->call.E, E, (size_t)n * d, ctx->stream));
    return dr_index_from_device_E(ctx, ctx->call.E.ptr(), n, d);
}

FDR_EXPORT int fdr_dense_index_embed(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr, const int32_t *a_indices) {
    int rc = use_device(ctx);
    if (rc) return rc;
    dr_index_reset(ctx->di);
    if ((rc = check_csr(n_rows, a_indptr, a_indices))) return rc;
    if (!ctx->proj.loaded()) return fail(FDR_E_STATE, "dense_index_embed: no projection loaded");
    if (n_rows < 1 || n_rows > INT32_MAX)
        return fail(FDR_E_ARG, "dense_index_embed: n_rows (%lld) must be in [1, 2^31)", (long long)n_rows);
    const int d = ctx->proj.d;
    if (d > FDR_FAST_MAX_DIM)
        return fail(FDR_E_ARG, "dense_index_embed: d = %d is outside [1, %d], the reach of the fp16 passes (the dense index "
                    "has no other path)", d, FDR_FAST_MAX_DIM);
    if ((rc = ctx->call.E.reserve((size_t)n_rows * d))) return rc;
    if ((rc = upload_embed_pipelined(ctx, n_rows, a_indptr, a_indices, ctx->call.E.ptr()))) return rc;
    return dr_index_from_device_E(ctx, ctx->call.E.ptr(), n_rows, d);
}

// what the two radius entries do first: no held result; the index, the radius, the cap
static int dr_radius_args(fdr_ctx *ctx, const char *who, float radius, int64_t max_hits) {
    ctx->di.rr.drop();
    return radius_args(ctx->di.valid, who, "dense", "fdr_knn", radius, max_hits);
}

// a call without queries: its figures, an empty result
static int dr_radius_none(DenseIndex &di, int64_t *indptr_out) {
    di.last_candidates = di.last_hits = 0;
    di.last_query_blocks = di.last_segments = 0;
    return radius_none(di.rr, indptr_out);
}

FDR_EXPORT int fdr_dense_index_radius_search(fdr_ctx *ctx, float radius, int64_t q_lo, int64_t q_hi, int64_t max_hits,
                                             int64_t *indptr_out) {
    static const char who[] = "dense_index_radius_search";
    int rc = use_device(ctx);
    if (rc) return rc;
    DenseIndex &di = ctx->di;
    if ((rc = dr_radius_args(ctx, who, radius, max_hits))) return rc;
    if (q_lo < 0 || q_hi < q_lo || q_hi > di.n)
        return fail(FDR_E_ARG, "%s: rows [%lld, %lld) are no range of the %lld rows", who, (long long)q_lo,
                    (long long)q_hi, (long long)di.n);
    if (!indptr_out) return fail(FDR_E_ARG, "%s: null pointer", who);
    const int64_t nq = q_hi - q_lo;
    if (nq == 0) return dr_radius_none(di, indptr_out);
    return dr_radius_passes(ctx, who, di.ehat.ptr() + (size_t)q_lo * di.dp, di.half.ptr() + (size_t)q_lo * di.dp,
                            di.zero.ptr() + q_lo, radius, nq, max_hits, indptr_out);
}

FDR_EXPORT int fdr_dense_index_radius_query(fdr_ctx *ctx, float radius, int64_t nq, const float *Q, int64_t max_hits,
                                            int64_t *indptr_out) {
    static const char who[] = "dense_index_radius_query";
    int rc = use_device(ctx);
    if (rc) return rc;
    DenseIndex &di = ctx->di;
    if ((rc = dr_radius_args(ctx, who, radius, max_hits))) return rc;
    if (nq < 0 || nq > INT32_MAX) return fail(FDR_E_ARG, "%s: nq (%lld) must be in [0, 2^31)", who, (long long)nq);
    if (!indptr_out) return fail(FDR_E_ARG, "%s: null pointer", who);
    if (nq == 0) return dr_radius_none(di, indptr_out);
    if (!Q) return fail(FDR_E_ARG, "%s: null pointer", who);
    const hipStream_t st = ctx->stream;
    // the queries go the index rows' way: the same upload, the same normalisation, the same fp16 conversion
    if ((rc = ctx->call.E.reserve((size_t)nq * di.d))) return rc;
    if ((rc = di.qhat.reserve((size_t)nq * di.dp))) return rc;
    if ((rc = di.qhalf.reserve((size_t)nq * di.dp))) return rc;
    if ((rc = di.qzero.reserve((size_t)nq))) return rc;
    HIP_TRY(upload(ctx->call.E, Q, (size_t)nq * di.d, st));
    if ((rc = launch_normalize(ctx, ctx->call.E.ptr(), nq, di.d, di.qhat.ptr(), di.qzero.ptr(), st))) return rc;
    hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)((nq * (di.dp / 8) + 255) / 256)), dim3(256), 0, st,
                       (const float *)di.qhat.ptr(), (long long)nq * (di.dp / 8), di.qhalf.ptr());
    HIP_TRY(hipGetLastError());
    return dr_radius_passes(ctx, who, di.qhat.ptr(), di.qhalf.ptr(), di.qzero.ptr(), radius, nq, max_hits, indptr_out);
}

FDR_EXPORT int fdr_dense_index_radius_fetch(fdr_ctx *ctx, int64_t hits, int32_t *idx_out, float *dist_out) {
    if (int rc = use_device(ctx)) return rc;
    return radius_fetch(ctx->stream, ctx->di.rr, "dense_index_radius_fetch", "next dense-index call", hits, idx_out, dist_out);
}

FDR_EXPORT int fdr_dense_index_info(fdr_ctx *ctx, int64_t *n, int32_t *d, size_t *device_bytes, int64_t *last_candidates,
                                    int64_t *last_hits, int32_t *last_query_blocks, int32_t *last_segments) {
    if (!ctx) return fail(FDR_E_ARG, "null context");
    DenseIndex &di = ctx->di;
    if (!di.valid) return fail(FDR_E_STATE, "dense_index_info: the context holds no dense index");
    if (n) *n = di.n;
    if (d) *d = di.d;
    if (device_bytes) *device_bytes = di.bytes();
    if (last_candidates) *last_candidates = di.last_candidates;
    if (last_hits) *last_hits = di.last_hits;
    if (last_query_blocks) *last_query_blocks = di.last_query_blocks;
    if (last_segments) *last_segments = di.last_segments;
    return FDR_OK;
}

FDR_EXPORT int fdr_dense_index_free(fdr_ctx *ctx) {
    int rc = use_device(ctx);
    if (rc) return rc;
    (void)hipStreamSynchronize(ctx->stream);
    ctx->di.release();
    return FDR_OK;
}
