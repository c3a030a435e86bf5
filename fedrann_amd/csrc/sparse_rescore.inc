// Part of libfedrann_hip.so (included by fedrann_hip.hip).
//
// fdr_sparse_rescore: candidate lists re-scored by exact distance on the sparse feature rows.  The projected search
// (fdr_embed_knn) names k_in rows per read in the projection's space; this call scores exactly those (query, candidate)
// pairs under a sparse metric of the feature rows and keeps the best k_out.  No postings, no sort of the entries, no
// table: both rows of a pair come from the one uploaded CSR, so a pair is the intersection of two ascending id lists.
//
// X1  rs_rows_kernel<METRIC>     one thread per row of the CSR, through sp_row<METRIC> (knn_sparse.inc), the device
//                                function of the index build's S1 / S1j / S1w: the argument checks, rinv and xhat =
//                                v * rinv (cosine), the set size and a "present" byte per entry where values are given
//                                (Jaccard), the mass chain (weighted Jaccard), the zero flag.  A row has the bits it has
//                                in an index build.  No posting keys, no run ids.
// X2  sparse_rescore_kernel<METRIC>  one wave (one workgroup) per query row.
//   check  the wave reads the query's k_in candidates into LDS; one outside [0, n) is recorded with one atomicMin as
//          (query row of the call << 8 | slot) and the wave scores nothing: the host reads the record (and X1's error
//          bits) back before it copies any result out.
//   score  the query's stored entries are staged in LDS, FDR_RESCORE_TILE at a time in ascending feature order (ids and
//          xhat / raw value / present mark), padded to a power of two with an id no entry holds.  Per tile a lane per
//          candidate first notes the candidate's stored entries for the tile (its row; nothing of a zero row); then the
//          candidates are taken in turn, a candidate's entries streamed in steps of RS_U chunks of 64, consecutive lanes
//          on consecutive entries, the next step's loads issued before the current step is searched (a wave has no
//          other work to hide them behind).  Each lane looks its RS_U features up in the tile by a binary search of
//          fixed length, the RS_U searches side by side.  The matches of a chunk are in ascending feature order by
//          lane, so the chain is continued by the wave chunk after chunk in lane order: acc <- fma(xhat_q, xhat_t, acc)
//          (cosine), m <- m + min(x_q, x_t) (weighted Jaccard), c <- c + popcount (Jaccard).  A query row longer than a
//          tile keeps the candidates' accumulators in LDS across its tiles and finds each candidate's slice for a tile
//          by binary search on the tile's first and last feature, so the order stays ascending over the whole row.  An
//          entry a build would give no posting contributes a zero term (cosine: xhat = +-0; weighted Jaccard: value
//          not > 0), which leaves the accumulator's bits alone, or is masked by its present mark (Jaccard).
//   rank   the distance of a pair of non-zero rows is sp_slot_dist<METRIC> of its accumulator (knn_sparse.inc: the
//          function S3 forms a table slot's distance with; cosine through dist_from_sim); two zero / empty / zero-mass
//          rows are at 0.0f, exactly one of them at 1.0f, and a pair that shares nothing comes out of the same
//          function at exactly 1.0f (c = 0: (a + b) / (a + b); m = +0; 1 - 0).  The k_in keys (distance bits << 32 |
//          index) are sorted by sp_bitonic and the first k_out written.
// So dist(q, t) is the float32 fdr_knn_sparse_metric reports for that pair on the same CSR whenever t is in q's list
// (DESIGN.md section 4: the chains, section 5: the argument).  The kernel takes a query's candidates as a pointer and a
// count (rs_score_row), so ragged lists of up to FDR_MAX_K candidates need no other kernel.
// Cost model: per pair the candidate's stored entries are read once per tile of the query: sum over the pairs of
// |row_t| * 4 bytes (Jaccard without values), 5 (with values) or 8 (cosine, weighted Jaccard), plus the upload of the CSR.

static_assert(FDR_RESCORE_TILE >= 64 && (FDR_RESCORE_TILE & (FDR_RESCORE_TILE - 1)) == 0, "a power of two of whole waves");
static_assert(FDR_MAX_K == 128, "the sort buffer holds 64 or 128 keys; a slot fits the refusal record's 8 bits");

template <int METRIC>
__global__ __launch_bounds__(256) void rs_rows_kernel(long long n, long long F, const long long *__restrict__ indptr,
                                                      const int *__restrict__ indices, const float *__restrict__ vals,
                                                      float *__restrict__ x, unsigned char *__restrict__ present,
                                                      int *__restrict__ asize, float *__restrict__ mass,
                                                      unsigned char *__restrict__ zero, u64 *__restrict__ cnt) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const SpRow r = sp_row<METRIC>(F, indices, vals, indptr[q], indptr[q + 1],
                                   [&](long long j, long long, float xv, bool) {
                                       if (METRIC != FDR_METRIC_JACCARD) x[j] = xv;
                                       else if (present) present[j] = xv != 0.0f ? 1 : 0;  // (Jaccard: xv is the value)
                                   });
    if (METRIC == FDR_METRIC_JACCARD) asize[q] = r.a;
    if (METRIC == FDR_METRIC_WEIGHTED_JACCARD) mass[q] = r.mass;
    zero[q] = r.zero ? 1 : 0;
    if (r.err) atomicOr(&cnt[RS_CNT_ERR], (u64)r.err);
}

// The rows of a re-score call on the device, as X1 leaves them
struct RsRows {
    const long long *indptr;       // [n + 1]
    const int *indices;            // the stored entries' features
    const float *x;                // cosine: xhat; weighted Jaccard: the raw values; Jaccard: null
    const unsigned char *present;  // Jaccard with values: 1 where the value is not +-0; otherwise null
    const int *asize;              // Jaccard: the set sizes
    const float *mass;             // weighted Jaccard: the masses
    const unsigned char *zero;     // the zero (empty, zero-mass) flags
};

// One wave scores query q against its kc <= FDR_MAX_K candidates cands[0, kc) (row numbers in [0, n), checked here) and
// writes the first k_out <= kc of them by (distance bits, index) to out_i / out_d.  `code` is the query's number in the
// refusal record.  LDS: qid / qx the query's tile (FDR_RESCORE_TILE each), cl the candidates, acc their accumulators,
// cb / ce their stored entries for the current tile (FDR_MAX_K each), keys the sort buffer (FDR_MAX_K; it may lie over
// the tile, which is dead by then).
constexpr int RS_U = 4;  // chunks of 64 stored entries of a candidate in flight per step
template <int METRIC>
__device__ __forceinline__ void rs_score_row(long long n, long long q, u64 code, const RsRows &rows,
                                             const int *__restrict__ cands, int kc, int k_out, int *qid, float *qx, int *cl,
                                             unsigned *acc, int *cb, int *ce, u64 *keys, u64 *__restrict__ cnt,
                                             int *__restrict__ out_i, float *__restrict__ out_d, int lane) {
    constexpr bool JAC = METRIC == FDR_METRIC_JACCARD;
    constexpr bool WJ = METRIC == FDR_METRIC_WEIGHTED_JACCARD;
    const long long *__restrict__ indptr = rows.indptr;
    const int *__restrict__ indices = rows.indices;
    const float *__restrict__ x = rows.x;
    const unsigned char *__restrict__ present = rows.present;
    // ---- check ----
    int bad = FDR_MAX_K;
    for (int s = lane; s < kc; s += 64) {
        const int t = cands[s];
        cl[s] = t;
        acc[s] = 0u;  // (+0.0f, or a count of 0)
        if ((t < 0 || t >= n) && bad == FDR_MAX_K) bad = s;
    }
    if (__ballot(bad != FDR_MAX_K)) {  // (wave-uniform)
        for (int off = 1; off < 64; off <<= 1) bad = min(bad, __shfl_xor(bad, off, 64));
        if (lane == 0) atomicMin(&cnt[RS_CNT_REFUSAL], (code << 8) | (u64)bad);
        return;
    }
    __syncthreads();
    // ---- score ----
    const long long qb = indptr[q], qe = indptr[q + 1];
    const bool qz = rows.zero[q] != 0;
    const bool multi = qe - qb > FDR_RESCORE_TILE;
    for (long long t0 = qb; t0 < qe && !qz; t0 += FDR_RESCORE_TILE) {
        const int tn = (int)min((long long)FDR_RESCORE_TILE, qe - t0);
        int P = 64;  // the tile padded to a power of two with ids no entry holds: a search of log2(P) fixed steps
        while (P < tn) P <<= 1;
        for (int i = lane; i < P; i += 64) {
            const bool in = i < tn;
            qid[i] = in ? indices[t0 + i] : INT32_MAX;
            qx[i] = !in ? 0.0f : JAC ? (present ? (float)present[t0 + i] : 1.0f) : x[t0 + i];
        }
        __syncthreads();
        // each candidate's stored entries for this tile, a lane per candidate: the whole row, or (a query of several
        // tiles) its entries with a feature in the tile's [f_lo, f_hi]; nothing of a zero row (the closed form)
        const int f_lo = qid[0], f_hi = qid[tn - 1];
        for (int s = lane; s < kc; s += 64) {
            const int t = cl[s];
            long long tb = 0, te = 0;
            if (!rows.zero[t]) {
                tb = indptr[t];
                te = indptr[t + 1];
                if (multi) {
                    const long long end = te;
                    tb = sp_lower_bound(indices, tb, end, f_lo);
                    te = sp_lower_bound(indices, tb, end, f_hi);
                    if (te < end && indices[te] == f_hi) ++te;
                }
            }
            cb[s] = (int)tb;  // (fewer than 2^31 stored entries)
            ce[s] = (int)te;
        }
        __syncthreads();
        // The walk: steps of RS_U * 64 entries of one candidate, the candidates in turn (all wave-uniform).  The loads
        // of the next step are issued before the current one is searched.
        auto advance = [&](int &s, long long &base, long long &end) {
            base += 64 * RS_U;
            while (base >= end) {
                if (++s >= kc) return;
                base = cb[s];
                end = ce[s];
            }
        };
        auto load = [&](long long base, long long end, int (&f)[RS_U], float (&v)[RS_U]) {
#pragma unroll
            for (int u = 0; u < RS_U; ++u) {
                const long long e = base + 64 * u + lane;
                const bool in = e < end;
                f[u] = in ? indices[e] : -1;
                if (JAC) v[u] = !in ? 0.0f : present ? (float)present[e] : 1.0f;
                else v[u] = in ? x[e] : 0.0f;
            }
        };
        int s = -1;
        long long base = 0, end = 0;
        advance(s, base, end);
        int fc[RS_U] = {}, fn[RS_U] = {};
        float vc[RS_U] = {}, vn[RS_U] = {};
        int c = 0;
        float a = 0.0f;
        if (s < kc) {
            load(base, end, fc, vc);
            c = (int)acc[s];
            a = __uint_as_float(acc[s]);
        }
        while (s < kc) {
            int ns = s;
            long long nbase = base, nend = end;
            advance(ns, nbase, nend);
            if (ns < kc) load(nbase, nend, fn, vn);
            int pos[RS_U] = {};
            for (int st = P >> 1; st > 0; st >>= 1) {
#pragma unroll
                for (int u = 0; u < RS_U; ++u)
                    if (qid[pos[u] + st - 1] < fc[u]) pos[u] += st;
            }
#pragma unroll
            for (int u = 0; u < RS_U; ++u) {  // (the chunks in turn: ascending features)
                const float vq = qx[pos[u]], vt = vc[u];
                bool hit = base + 64 * u + lane < end && pos[u] < tn && qid[pos[u]] == fc[u];
                if (JAC) hit = hit && vq != 0.0f && vt != 0.0f;
                u64 m = __ballot(hit);
                if (JAC) {
                    c += __popcll(m);
                } else {
                    while (m) {  // the chunk's shared features in ascending order (wave-uniform)
                        const int src = __builtin_ctzll(m);
                        m &= m - 1;
                        const float uq = __shfl(vq, src), ut = __shfl(vt, src);
                        a = WJ ? a + fminf(uq, ut) : __builtin_fmaf(uq, ut, a);
                    }
                }
            }
            if (ns != s) {  // (a candidate is walked once per tile: its slot is read and written by this step alone)
                if (lane == 0) acc[s] = JAC ? (unsigned)c : __float_as_uint(a);
                if (ns < kc) {
                    c = (int)acc[ns];
                    a = __uint_as_float(acc[ns]);
                }
            }
            s = ns;
            base = nbase;
            end = nend;
#pragma unroll
            for (int u = 0; u < RS_U; ++u) {
                fc[u] = fn[u];
                vc[u] = vn[u];
            }
        }
        __syncthreads();  // (the accumulators are written, the tile is read: the next tile may take its place)
    }
    // ---- rank ----
    const int qa = JAC ? rows.asize[q] : 0;                 // |S_q|
    const double qm = WJ ? (double)rows.mass[q] : 0.0;      // A_q
    const int P = kc <= 64 ? 64 : FDR_MAX_K;
    for (int s = lane; s < P; s += 64) {
        u64 key = ~0ull;
        if (s < kc) {
            const int t = cl[s];
            const bool tz = rows.zero[t] != 0;
            float d;
            if (qz || tz) d = qz && tz ? 0.0f : 1.0f;
            else d = sp_slot_dist<METRIC>(((u64)acc[s] << 32) | (unsigned)t, t, qa, qm, rows.asize, rows.mass);
            key = ((u64)__float_as_uint(d) << 32) | (unsigned)t;
        }
        keys[s] = key;
    }
    __syncthreads();
    sp_bitonic(keys, P, lane);
    for (int i = lane; i < k_out; i += 64) {
        const u64 key = keys[i];
        out_i[i] = (int)(unsigned)key;
        out_d[i] = __uint_as_float((unsigned)(key >> 32));
    }
}

// X2: workgroup r takes query q_lo + r, its candidates cand[r * k_in, (r + 1) * k_in) and row r of the results
template <int METRIC>
__global__ __launch_bounds__(64) void sparse_rescore_kernel(long long n, long long q_lo, int k_in, int k_out,
                                                            const RsRows rows, const int *__restrict__ cand,
                                                            u64 *__restrict__ cnt, int *__restrict__ idx_out,
                                                            float *__restrict__ dist_out) {
    __shared__ u64 tile[FDR_RESCORE_TILE / 2];  // the query's ids (int32); in the end the sort buffer
    __shared__ float qx[FDR_RESCORE_TILE];
    __shared__ int cl[FDR_MAX_K], cb[FDR_MAX_K], ce[FDR_MAX_K];
    __shared__ unsigned acc[FDR_MAX_K];
    static_assert(FDR_RESCORE_TILE / 2 >= FDR_MAX_K, "the sort buffer fits the tile");
    const long long r = blockIdx.x;
    rs_score_row<METRIC>(n, q_lo + r, (u64)r, rows, cand + r * k_in, k_in, k_out, reinterpret_cast<int *>(tile), qx, cl,
                         acc, cb, ce, tile, cnt, idx_out + r * k_out, dist_out + r * k_out, (int)threadIdx.x);
}

template <int METRIC>
static void rs_launch(fdr_ctx *ctx, int64_t n, int64_t n_features, bool has_values, int64_t q_lo, int64_t nq, int32_t k_in,
                      int32_t k_out) {
    constexpr bool JAC = METRIC == FDR_METRIC_JACCARD;
    constexpr bool WJ = METRIC == FDR_METRIC_WEIGHTED_JACCARD;
    SparseRescoreScratch &rs = ctx->rs;
    const hipStream_t st = ctx->stream;
    float *x = JAC ? nullptr : rs.x.ptr();
    unsigned char *present = JAC && has_values ? rs.present.ptr() : nullptr;
    int *asize = JAC ? rs.asize.ptr() : nullptr;
    float *mass = WJ ? rs.mass.ptr() : nullptr;
    hipLaunchKernelGGL((rs_rows_kernel<METRIC>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n,
                       (long long)n_features, rs.indptr.ptr(), rs.indices.ptr(), has_values ? rs.values.ptr() : nullptr, x,
                       present, asize, mass, rs.zero.ptr(), rs.cnt.ptr());
    const RsRows rows = {rs.indptr.ptr(), rs.indices.ptr(), x, present, asize, mass, rs.zero.ptr()};
    hipLaunchKernelGGL((sparse_rescore_kernel<METRIC>), dim3((unsigned)nq), dim3(64), 0, st, (long long)n,
                       (long long)q_lo, (int)k_in, (int)k_out, rows, rs.cand.ptr(), rs.cnt.ptr(), rs.idx_out.ptr(),
                       rs.dist_out.ptr());
}

FDR_EXPORT int fdr_sparse_rescore(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features, const int64_t *indptr,
                                  const int32_t *indices, const float *values, int64_t q_lo, int64_t nq, int32_t k_in,
                                  const int32_t *cand_idx, int32_t k_out, int32_t *idx_out, float *dist_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    const bool jac = metric == FDR_METRIC_JACCARD, wj = metric == FDR_METRIC_WEIGHTED_JACCARD;
    if (!jac && !wj && metric != FDR_METRIC_COSINE)
        return fail(FDR_E_ARG, "sparse_rescore: unknown metric %d (FDR_METRIC_COSINE, FDR_METRIC_JACCARD, "
                    "FDR_METRIC_WEIGHTED_JACCARD)", metric);
    if (k_in < 1 || k_in > FDR_MAX_K)
        return fail(FDR_E_ARG, "sparse_rescore: k_in=%d unsupported (1..%d)", k_in, FDR_MAX_K);
    if (k_out < 1 || k_out > k_in)
        return fail(FDR_E_ARG, "sparse_rescore: k_out=%d unsupported (1..k_in = %d)", k_out, k_in);
    if (n < 1) return fail(FDR_E_ARG, "sparse_rescore: need at least one row, got n = %lld", (long long)n);
    if (n > INT32_MAX) return fail(FDR_E_ARG, "sparse_rescore: n (%lld) must be below 2^31 rows", (long long)n);
    if (n_features < 1 || n_features > INT32_MAX)
        return fail(FDR_E_ARG, "sparse_rescore: n_features (%lld) must be in [1, 2^31)", (long long)n_features);
    if (q_lo < 0 || nq < 0 || q_lo > n || nq > n - q_lo)
        return fail(FDR_E_ARG, "sparse_rescore: queries [%lld, %lld + %lld) are no range of the %lld rows", (long long)q_lo,
                    (long long)q_lo, (long long)nq, (long long)n);
    if (nq * k_in > INT32_MAX)
        return fail(FDR_E_ARG, "sparse_rescore: %lld queries of %d candidates: an array of 2^31 elements or more",
                    (long long)nq, k_in);
    if (nq == 0) return FDR_OK;
    if (!indptr || !cand_idx || !idx_out || !dist_out) return fail(FDR_E_ARG, "sparse_rescore: null pointer");
    if (indptr[0] != 0) return fail(FDR_E_ARG, "sparse_rescore: indptr[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i])
            return fail(FDR_E_ARG, "sparse_rescore: indptr not monotone at row %lld", (long long)i);
    const int64_t nnz = indptr[n];
    if (nnz > INT32_MAX)
        return fail(FDR_E_ARG, "sparse_rescore: %lld stored entries (at most 2^31 - 1)", (long long)nnz);
    if (nnz > 0 && !indices) return fail(FDR_E_ARG, "sparse_rescore: indices is null");
    SparseRescoreScratch &rs = ctx->rs;
    const hipStream_t st = ctx->stream;
    const size_t m1 = (size_t)std::max<int64_t>(nnz, 1), n_in = (size_t)nq * (size_t)k_in, n_out = (size_t)nq * (size_t)k_out;
    if ((rc = rs.indptr.reserve((size_t)(n + 1)))) return rc;
    if ((rc = rs.indices.reserve(m1))) return rc;
    if (values && (rc = rs.values.reserve(m1))) return rc;
    if (!jac && (rc = rs.x.reserve(m1))) return rc;
    if (jac && values && (rc = rs.present.reserve(m1))) return rc;
    if (jac && (rc = rs.asize.reserve((size_t)n))) return rc;
    if (wj && (rc = rs.mass.reserve((size_t)n))) return rc;
    if ((rc = rs.zero.reserve((size_t)n))) return rc;
    if ((rc = rs.cand.reserve(n_in))) return rc;
    if ((rc = rs.idx_out.reserve(n_out))) return rc;
    if ((rc = rs.dist_out.reserve(n_out))) return rc;
    if ((rc = rs.cnt.reserve(RS_CNT_WORDS))) return rc;
    HIP_TRY(hipMemcpyAsync(rs.indptr.ptr(), indptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        HIP_TRY(hipMemcpyAsync(rs.indices.ptr(), indices, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        if (values) HIP_TRY(hipMemcpyAsync(rs.values.ptr(), values, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(rs.cand.ptr(), cand_idx, n_in * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(rs.cnt.ptr() + RS_CNT_ERR, 0, 8, st));
    HIP_TRY(hipMemsetAsync(rs.cnt.ptr() + RS_CNT_REFUSAL, 0xff, 8, st));
    if (jac) rs_launch<FDR_METRIC_JACCARD>(ctx, n, n_features, values != nullptr, q_lo, nq, k_in, k_out);
    else if (wj) rs_launch<FDR_METRIC_WEIGHTED_JACCARD>(ctx, n, n_features, values != nullptr, q_lo, nq, k_in, k_out);
    else rs_launch<FDR_METRIC_COSINE>(ctx, n, n_features, values != nullptr, q_lo, nq, k_in, k_out);
    HIP_TRY(hipGetLastError());
    u64 h[RS_CNT_WORDS] = {0, 0};  // the rows' error bits; the refusal record
    HIP_TRY(hipMemcpyAsync(h, rs.cnt.ptr(), sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (nothing has been written to idx_out / dist_out)
    if ((rc = sp_refuse("sparse_rescore", h[RS_CNT_ERR], n_features))) return rc;
    if (h[RS_CNT_REFUSAL] != ~0ull) {
        const long long row = (long long)(h[RS_CNT_REFUSAL] >> 8);
        const int slot = (int)(h[RS_CNT_REFUSAL] & 0xff);
        return fail(FDR_E_ARG, "sparse_rescore: query %lld, slot %d: the candidate (%d) is no row in [0, %lld)",
                    (long long)q_lo + row, slot, cand_idx[(size_t)row * (size_t)k_in + (size_t)slot], (long long)n);
    }
    HIP_TRY(download(idx_out, rs.idx_out, n_out, st));
    HIP_TRY(download(dist_out, rs.dist_out, n_out, st));
    HIP_TRY(hipStreamSynchronize(st));
    return FDR_OK;
}
