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
// (DESIGN.md section 4: the chains, section 5: the argument).
// X3  sparse_rescore_ragged_kernel<METRIC>  one wave (one workgroup) per (query, batch of at most FDR_MAX_K consecutive
//          candidates of its ragged row): check and score are X2's functions, so a pair's chain depends on its two
//          rows alone; rank stores each candidate's key at its own place of the input segment and counts the keys
//          within the radius.  The held row set's calls (fdr_rescore_rows_*, below) run it inside the radius
//          searches' frame: one segmented sort over the input segments, the hits compacted from their heads.
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

// The phases of a wave that scores query q against kc <= FDR_MAX_K candidates, for X2 (a query's whole list) and X3 (a
// batch of a ragged row): check and score are shared, so a pair's chain depends on its two rows alone, and each kernel
// ranks in its own way from rs_pair_key.  LDS: qid / qx the query's tile (FDR_RESCORE_TILE each), cl the candidates,
// acc their accumulators, cb / ce their stored entries for the current tile (FDR_MAX_K each).
constexpr int RS_U = 4;  // chunks of 64 stored entries of a candidate in flight per step

// check: cands[0, kc) -> cl, the accumulators cleared.  Returns (wave-uniform) the first slot whose candidate is no
// row in [0, n), or FDR_MAX_K: then the caller passes a barrier and scores.
__device__ __forceinline__ int rs_check(long long n, const int *__restrict__ cands, int kc, int *cl, unsigned *acc,
                                        int lane) {
    int bad = FDR_MAX_K;
    for (int s = lane; s < kc; s += 64) {
        const int t = cands[s];
        cl[s] = t;
        acc[s] = 0u;  // (+0.0f, or a count of 0)
        if ((t < 0 || t >= n) && bad == FDR_MAX_K) bad = s;
    }
    if (__ballot(bad != FDR_MAX_K))  // (wave-uniform)
        for (int off = 1; off < 64; off <<= 1) bad = min(bad, __shfl_xor(bad, off, 64));
    return bad;
}

// score: acc[s] <- the chain of (q, cl[s]) over the features both rows hold, for the kc candidates (see the head)
template <int METRIC>
__device__ __forceinline__ void rs_score(long long q, const RsRows &rows, int kc, int *qid, float *qx, const int *cl,
                                         unsigned *acc, int *cb, int *ce, int lane) {
    constexpr bool JAC = METRIC == FDR_METRIC_JACCARD;
    constexpr bool WJ = METRIC == FDR_METRIC_WEIGHTED_JACCARD;
    const long long *__restrict__ indptr = rows.indptr;
    const int *__restrict__ indices = rows.indices;
    const float *__restrict__ x = rows.x;
    const unsigned char *__restrict__ present = rows.present;
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
}

// What the rank phase knows of the query, and the key (distance bits << 32 | index) of its pair with candidate t whose
// accumulator rs_score left as `a`
struct RsQuery {
    bool zero;
    int asize;    // |S_q| (Jaccard)
    double mass;  // A_q (weighted Jaccard)
};
template <int METRIC>
__device__ __forceinline__ RsQuery rs_query(long long q, const RsRows &rows) {
    return RsQuery{rows.zero[q] != 0, METRIC == FDR_METRIC_JACCARD ? rows.asize[q] : 0,
                   METRIC == FDR_METRIC_WEIGHTED_JACCARD ? (double)rows.mass[q] : 0.0};
}
template <int METRIC>
__device__ __forceinline__ u64 rs_pair_key(const RsQuery &qr, const RsRows &rows, int t, unsigned a) {
    const bool tz = rows.zero[t] != 0;
    float d;
    if (qr.zero || tz) d = qr.zero && tz ? 0.0f : 1.0f;
    else d = sp_slot_dist<METRIC>(((u64)a << 32) | (unsigned)t, t, qr.asize, qr.mass, rows.asize, rows.mass);
    return ((u64)__float_as_uint(d) << 32) | (unsigned)t;
}

// One wave scores query q against its kc <= FDR_MAX_K candidates cands[0, kc) (row numbers in [0, n), checked here) and
// writes the first k_out <= kc of them by (distance bits, index) to out_i / out_d.  `code` is the query's number in the
// refusal record.  keys: the sort buffer (FDR_MAX_K; it may lie over the tile, which is dead by then).
template <int METRIC>
__device__ __forceinline__ void rs_score_row(long long n, long long q, u64 code, const RsRows &rows,
                                             const int *__restrict__ cands, int kc, int k_out, int *qid, float *qx, int *cl,
                                             unsigned *acc, int *cb, int *ce, u64 *keys, u64 *__restrict__ cnt,
                                             int *__restrict__ out_i, float *__restrict__ out_d, int lane) {
    const int bad = rs_check(n, cands, kc, cl, acc, lane);
    if (bad != FDR_MAX_K) {  // (the wave scores nothing)
        if (lane == 0) atomicMin(&cnt[RS_CNT_REFUSAL], (code << 8) | (u64)bad);
        return;
    }
    __syncthreads();
    rs_score<METRIC>(q, rows, kc, qid, qx, cl, acc, cb, ce, lane);
    // ---- rank ----
    const RsQuery qr = rs_query<METRIC>(q, rows);
    const int P = kc <= 64 ? 64 : FDR_MAX_K;
    for (int s = lane; s < P; s += 64) keys[s] = s < kc ? rs_pair_key<METRIC>(qr, rows, cl[s], acc[s]) : ~0ull;
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

// X3: workgroup i takes the work item items[i] = (query row r of the call, batch b): the candidates [FDR_MAX_K * b,
// FDR_MAX_K * (b + 1)) of the row cand[cand_indptr[r], cand_indptr[r + 1]), as far as it reaches (the host lists only
// batches that hold a candidate).  check and score as X2; rank: every candidate's key goes to its own place of the
// segment in `keys`, and the keys with distance bits <= rbits are added to count[r] with one atomic.  A candidate
// outside [0, n) is recorded as (r << 32 | position in the row) and the item writes nothing.
template <int METRIC>
__global__ __launch_bounds__(64) void sparse_rescore_ragged_kernel(long long n, long long q_lo, unsigned rbits,
                                                                   const RsRows rows, const int2 *__restrict__ items,
                                                                   const long long *__restrict__ cand_indptr,
                                                                   const int *__restrict__ cand, u64 *__restrict__ cnt,
                                                                   u64 *__restrict__ keys,
                                                                   unsigned long long *__restrict__ count) {
    __shared__ int qid[FDR_RESCORE_TILE];
    __shared__ float qx[FDR_RESCORE_TILE];
    __shared__ int cl[FDR_MAX_K], cb[FDR_MAX_K], ce[FDR_MAX_K];
    __shared__ unsigned acc[FDR_MAX_K];
    const int lane = (int)threadIdx.x;
    const int2 it = items[blockIdx.x];
    const long long r = it.x, pos0 = (long long)it.y * FDR_MAX_K;
    const long long seg0 = cand_indptr[r] + pos0;
    const int kc = (int)min((long long)FDR_MAX_K, cand_indptr[r + 1] - seg0);
    const long long q = q_lo + r;
    const int bad = rs_check(n, cand + seg0, kc, cl, acc, lane);
    if (bad != FDR_MAX_K) {
        if (lane == 0) atomicMin(&cnt[RS_CNT_REFUSAL], ((u64)r << 32) | (u64)(pos0 + bad));
        return;
    }
    __syncthreads();
    rs_score<METRIC>(q, rows, kc, qid, qx, cl, acc, cb, ce, lane);
    // ---- rank ----
    const RsQuery qr = rs_query<METRIC>(q, rows);
    int hits = 0;
    for (int s0 = 0; s0 < kc; s0 += 64) {  // (wave-uniform trips: the ballot sees every lane)
        const int s = s0 + lane;
        bool hit = false;
        if (s < kc) {
            const u64 key = rs_pair_key<METRIC>(qr, rows, cl[s], acc[s]);
            keys[seg0 + s] = key;
            hit = (unsigned)(key >> 32) <= rbits;  // (non-negative floats: bit order is value order)
        }
        hits += __popcll(__ballot(hit));
    }
    if (lane == 0 && hits) atomicAdd(count + r, (unsigned long long)hits);
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The checks fdr_sparse_rescore and the held row set's calls make alike; `who` is the entry point's name in messages.
static int rs_check_metric(const char *who, int32_t metric) {
    if (metric != FDR_METRIC_JACCARD && metric != FDR_METRIC_WEIGHTED_JACCARD && metric != FDR_METRIC_COSINE)
        return fail(FDR_E_ARG, "%s: unknown metric %d (FDR_METRIC_COSINE, FDR_METRIC_JACCARD, "
                    "FDR_METRIC_WEIGHTED_JACCARD)", who, metric);
    return FDR_OK;
}
static int rs_check_k(const char *who, int32_t k_in, int32_t k_out) {
    if (k_in < 1 || k_in > FDR_MAX_K) return fail(FDR_E_ARG, "%s: k_in=%d unsupported (1..%d)", who, k_in, FDR_MAX_K);
    if (k_out < 1 || k_out > k_in) return fail(FDR_E_ARG, "%s: k_out=%d unsupported (1..k_in = %d)", who, k_out, k_in);
    return FDR_OK;
}
static int rs_check_shape(const char *who, int64_t n, int64_t n_features) {
    if (n < 1) return fail(FDR_E_ARG, "%s: need at least one row, got n = %lld", who, (long long)n);
    if (n > INT32_MAX) return fail(FDR_E_ARG, "%s: n (%lld) must be below 2^31 rows", who, (long long)n);
    if (n_features < 1 || n_features > INT32_MAX)
        return fail(FDR_E_ARG, "%s: n_features (%lld) must be in [1, 2^31)", who, (long long)n_features);
    return FDR_OK;
}
static int rs_check_queries(const char *who, int64_t n, int64_t q_lo, int64_t nq) {
    if (q_lo < 0 || nq < 0 || q_lo > n || nq > n - q_lo)
        return fail(FDR_E_ARG, "%s: queries [%lld, %lld + %lld) are no range of the %lld rows", who, (long long)q_lo,
                    (long long)q_lo, (long long)nq, (long long)n);
    return FDR_OK;
}
static int rs_check_list_total(const char *who, int64_t nq, int32_t k_in) {
    if (nq * k_in > INT32_MAX)
        return fail(FDR_E_ARG, "%s: %lld queries of %d candidates: an array of 2^31 elements or more", who, (long long)nq,
                    k_in);
    return FDR_OK;
}
// the CSR's row pointer; *nnz: the stored entries
static int rs_check_indptr(const char *who, int64_t n, const int64_t *indptr, const int32_t *indices, int64_t *nnz) {
    if (indptr[0] != 0) return fail(FDR_E_ARG, "%s: indptr[0] must be 0", who);
    for (int64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(FDR_E_ARG, "%s: indptr not monotone at row %lld", who, (long long)i);
    *nnz = indptr[n];
    if (*nnz > INT32_MAX) return fail(FDR_E_ARG, "%s: %lld stored entries (at most 2^31 - 1)", who, (long long)*nnz);
    if (*nnz > 0 && !indices) return fail(FDR_E_ARG, "%s: indices is null", who);
    return FDR_OK;
}

// room for a CSR of n rows and nnz stored entries under `metric`, and for what X1 makes of it
static int rs_csr_reserve(RsCsr &c, int32_t metric, int64_t n, int64_t nnz, bool has_values) {
    int rc;
    const bool jac = metric == FDR_METRIC_JACCARD, wj = metric == FDR_METRIC_WEIGHTED_JACCARD;
    const size_t m1 = (size_t)std::max<int64_t>(nnz, 1);
    if ((rc = c.indptr.reserve((size_t)(n + 1)))) return rc;
    if ((rc = c.indices.reserve(m1))) return rc;
    if (has_values && (rc = c.values.reserve(m1))) return rc;
    if (!jac && (rc = c.x.reserve(m1))) return rc;
    if (jac && has_values && (rc = c.present.reserve(m1))) return rc;
    if (jac && (rc = c.asize.reserve((size_t)n))) return rc;
    if (wj && (rc = c.mass.reserve((size_t)n))) return rc;
    return c.zero.reserve((size_t)n);
}
static int rs_csr_upload(RsCsr &c, hipStream_t st, int64_t n, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                         const float *values) {
    HIP_TRY(hipMemcpyAsync(c.indptr.ptr(), indptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        HIP_TRY(hipMemcpyAsync(c.indices.ptr(), indices, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        if (values) HIP_TRY(hipMemcpyAsync(c.values.ptr(), values, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    }
    return FDR_OK;
}
// the rows of a reserved CSR as the kernels take them (what a metric does not use is null)
static RsRows rs_rows_of(const RsCsr &c, int32_t metric, bool has_values) {
    const bool jac = metric == FDR_METRIC_JACCARD, wj = metric == FDR_METRIC_WEIGHTED_JACCARD;
    return RsRows{c.indptr.ptr(), c.indices.ptr(), jac ? nullptr : c.x.ptr(), jac && has_values ? c.present.ptr() : nullptr,
                  jac ? c.asize.ptr() : nullptr, wj ? c.mass.ptr() : nullptr, c.zero.ptr()};
}

// X1 over an uploaded CSR; the rows' error bits are or-ed into cnt[RS_CNT_ERR]
template <int METRIC>
static void rs_x1_launch(RsCsr &c, hipStream_t st, int64_t n, int64_t n_features, bool has_values, u64 *cnt) {
    const RsRows r = rs_rows_of(c, METRIC, has_values);
    hipLaunchKernelGGL((rs_rows_kernel<METRIC>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n,
                       (long long)n_features, c.indptr.ptr(), c.indices.ptr(), has_values ? c.values.ptr() : nullptr,
                       const_cast<float *>(r.x), const_cast<unsigned char *>(r.present), const_cast<int *>(r.asize),
                       const_cast<float *>(r.mass), c.zero.ptr(), cnt);
}
static void rs_x1(RsCsr &c, hipStream_t st, int32_t metric, int64_t n, int64_t n_features, bool has_values, u64 *cnt) {
    if (metric == FDR_METRIC_JACCARD) rs_x1_launch<FDR_METRIC_JACCARD>(c, st, n, n_features, has_values, cnt);
    else if (metric == FDR_METRIC_WEIGHTED_JACCARD) rs_x1_launch<FDR_METRIC_WEIGHTED_JACCARD>(c, st, n, n_features, has_values, cnt);
    else rs_x1_launch<FDR_METRIC_COSINE>(c, st, n, n_features, has_values, cnt);
}

// The rectangular lists of a call, in three steps.  begin: room, the candidates' upload, both counter words cleared.
static int rs_lists_begin(RsLists &l, hipStream_t st, const int32_t *cand_idx, size_t n_in, size_t n_out) {
    int rc;
    if ((rc = l.cand.reserve(n_in))) return rc;
    if ((rc = l.idx_out.reserve(n_out))) return rc;
    if ((rc = l.dist_out.reserve(n_out))) return rc;
    if ((rc = l.cnt.reserve(RS_CNT_WORDS))) return rc;
    HIP_TRY(hipMemcpyAsync(l.cand.ptr(), cand_idx, n_in * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(l.cnt.ptr() + RS_CNT_ERR, 0, 8, st));
    HIP_TRY(hipMemsetAsync(l.cnt.ptr() + RS_CNT_REFUSAL, 0xff, 8, st));
    return FDR_OK;
}
// X2 over the lists
template <int METRIC>
static void rs_x2_launch(RsLists &l, hipStream_t st, const RsRows &rows, int64_t n, int64_t q_lo, int64_t nq, int32_t k_in,
                         int32_t k_out) {
    hipLaunchKernelGGL((sparse_rescore_kernel<METRIC>), dim3((unsigned)nq), dim3(64), 0, st, (long long)n,
                       (long long)q_lo, (int)k_in, (int)k_out, rows, l.cand.ptr(), l.cnt.ptr(), l.idx_out.ptr(),
                       l.dist_out.ptr());
}
static void rs_x2(RsLists &l, hipStream_t st, int32_t metric, const RsRows &rows, int64_t n, int64_t q_lo, int64_t nq,
                  int32_t k_in, int32_t k_out) {
    if (metric == FDR_METRIC_JACCARD) rs_x2_launch<FDR_METRIC_JACCARD>(l, st, rows, n, q_lo, nq, k_in, k_out);
    else if (metric == FDR_METRIC_WEIGHTED_JACCARD) rs_x2_launch<FDR_METRIC_WEIGHTED_JACCARD>(l, st, rows, n, q_lo, nq, k_in, k_out);
    else rs_x2_launch<FDR_METRIC_COSINE>(l, st, rows, n, q_lo, nq, k_in, k_out);
}
// end: the counters read back, the rows' errors and a candidate outside [0, n) refused before anything is copied out
static int rs_lists_end(RsLists &l, hipStream_t st, const char *who, int64_t n, int64_t n_features, int64_t q_lo,
                        int32_t k_in, const int32_t *cand_idx, size_t n_out, int32_t *idx_out, float *dist_out) {
    int rc;
    HIP_TRY(hipGetLastError());
    u64 h[RS_CNT_WORDS] = {0, 0};  // the rows' error bits; the refusal record
    HIP_TRY(hipMemcpyAsync(h, l.cnt.ptr(), sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (nothing has been written to idx_out / dist_out)
    if ((rc = sp_refuse(who, h[RS_CNT_ERR], n_features))) return rc;
    if (h[RS_CNT_REFUSAL] != ~0ull) {
        const long long row = (long long)(h[RS_CNT_REFUSAL] >> 8);
        const int slot = (int)(h[RS_CNT_REFUSAL] & 0xff);
        return fail(FDR_E_ARG, "%s: query %lld, slot %d: the candidate (%d) is no row in [0, %lld)", who,
                    (long long)q_lo + row, slot, cand_idx[(size_t)row * (size_t)k_in + (size_t)slot], (long long)n);
    }
    HIP_TRY(download(idx_out, l.idx_out, n_out, st));
    HIP_TRY(download(dist_out, l.dist_out, n_out, st));
    HIP_TRY(hipStreamSynchronize(st));
    return FDR_OK;
}

FDR_EXPORT int fdr_sparse_rescore(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features, const int64_t *indptr,
                                  const int32_t *indices, const float *values, int64_t q_lo, int64_t nq, int32_t k_in,
                                  const int32_t *cand_idx, int32_t k_out, int32_t *idx_out, float *dist_out) {
    static const char who[] = "sparse_rescore";
    int rc = use_device(ctx);
    if (rc) return rc;
    if ((rc = rs_check_metric(who, metric))) return rc;
    if ((rc = rs_check_k(who, k_in, k_out))) return rc;
    if ((rc = rs_check_shape(who, n, n_features))) return rc;
    if ((rc = rs_check_queries(who, n, q_lo, nq))) return rc;
    if ((rc = rs_check_list_total(who, nq, k_in))) return rc;
    if (nq == 0) return FDR_OK;
    if (!indptr || !cand_idx || !idx_out || !dist_out) return fail(FDR_E_ARG, "%s: null pointer", who);
    int64_t nnz = 0;
    if ((rc = rs_check_indptr(who, n, indptr, indices, &nnz))) return rc;
    SparseRescoreScratch &rs = ctx->rs;
    const hipStream_t st = ctx->stream;
    const size_t n_in = (size_t)nq * (size_t)k_in, n_out = (size_t)nq * (size_t)k_out;
    if ((rc = rs_csr_reserve(rs.csr, metric, n, nnz, values != nullptr))) return rc;
    if ((rc = rs_csr_upload(rs.csr, st, n, nnz, indptr, indices, values))) return rc;
    if ((rc = rs_lists_begin(rs.lists, st, cand_idx, n_in, n_out))) return rc;
    rs_x1(rs.csr, st, metric, n, n_features, values != nullptr, rs.lists.cnt.ptr());
    rs_x2(rs.lists, st, metric, rs_rows_of(rs.csr, metric, values != nullptr), n, q_lo, nq, k_in, k_out);
    return rs_lists_end(rs.lists, st, who, n, n_features, q_lo, k_in, cand_idx, n_out, idx_out, dist_out);
}

// ---- the held row set -----------------------------------------------------------------------------------------------
// fdr_rescore_rows_*: X1 once at the build; X2 (_knn) and X3 (_radius) on the rows it left.  _radius runs the radius
// searches' frame (knn_radius_common.inc) on the row set's RadiusResult with the CANDIDATES' segments as the sort's:
// X3 leaves every candidate's key in its place and the hits' number per query; the scan of those is indptr_out; one
// segmented sort orders every segment by (distance bits, index), so a query's hits are the first count[q] keys of its
// segment, and radius_split_kernel<true> compacts them into the result.  Every pair is scored once: there is no
// second pass and so no cross-check.
static const char rr_next[] = "next fdr_rescore_rows_ call other than _info and _knn";

FDR_EXPORT int fdr_rescore_rows_build(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features, const int64_t *indptr,
                                      const int32_t *indices, const float *values) {
    static const char who[] = "rescore_rows_build";
    int rc = use_device(ctx);
    if (rc) return rc;
    RescoreRowSet &s = ctx->rrs;
    s.valid = false;  // (a refused or failed build leaves no row set)
    s.rr.drop();
    if ((rc = rs_check_metric(who, metric))) return rc;
    if ((rc = rs_check_shape(who, n, n_features))) return rc;
    if (!indptr) return fail(FDR_E_ARG, "%s: null pointer", who);
    int64_t nnz = 0;
    if ((rc = rs_check_indptr(who, n, indptr, indices, &nnz))) return rc;
    const hipStream_t st = ctx->stream;
    const bool has_values = values != nullptr;
    // what this metric does not use goes: a set built under another metric does not stay in device_bytes
    HIP_TRY(hipStreamSynchronize(st));
    if (metric == FDR_METRIC_JACCARD) s.csr.x.release();
    else release_all(s.csr.asize, s.csr.present);
    if (metric == FDR_METRIC_JACCARD && !has_values) s.csr.present.release();
    if (metric != FDR_METRIC_WEIGHTED_JACCARD) s.csr.mass.release();
    if ((rc = rs_csr_reserve(s.csr, metric, n, nnz, has_values))) return rc;
    if ((rc = s.lists.cnt.reserve(RS_CNT_WORDS))) return rc;
    if ((rc = rs_csr_upload(s.csr, st, n, nnz, indptr, indices, values))) return rc;
    HIP_TRY(hipMemsetAsync(s.lists.cnt.ptr() + RS_CNT_ERR, 0, 8, st));
    rs_x1(s.csr, st, metric, n, n_features, has_values, s.lists.cnt.ptr());
    HIP_TRY(hipGetLastError());
    u64 err = 0;
    HIP_TRY(hipMemcpyAsync(&err, s.lists.cnt.ptr() + RS_CNT_ERR, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = sp_refuse(who, err, n_features))) return rc;
    s.csr.values.release();  // (X1 has read them: x / present hold what the kernels need)
    s.metric = metric;
    s.n = n;
    s.stored = nnz;
    s.has_values = has_values;
    s.valid = true;
    return FDR_OK;
}

FDR_EXPORT int fdr_rescore_rows_info(fdr_ctx *ctx, int32_t *metric, int64_t *n, int64_t *stored, size_t *device_bytes) {
    if (!ctx) return fail(FDR_E_ARG, "null context");
    RescoreRowSet &s = ctx->rrs;
    if (!s.valid) return fail(FDR_E_STATE, "rescore_rows_info: the context holds no re-score rows");
    if (metric) *metric = s.metric;
    if (n) *n = s.n;
    if (stored) *stored = s.stored;
    if (device_bytes) *device_bytes = s.bytes();
    return FDR_OK;
}

FDR_EXPORT int fdr_rescore_rows_free(fdr_ctx *ctx) {
    int rc = use_device(ctx);
    if (rc) return rc;
    (void)hipStreamSynchronize(ctx->stream);
    ctx->rrs.release();
    return FDR_OK;
}

FDR_EXPORT int fdr_rescore_rows_knn(fdr_ctx *ctx, int64_t q_lo, int64_t nq, int32_t k_in, const int32_t *cand_idx,
                                    int32_t k_out, int32_t *idx_out, float *dist_out) {
    static const char who[] = "rescore_rows_knn";
    int rc = use_device(ctx);
    if (rc) return rc;
    RescoreRowSet &s = ctx->rrs;
    if (!s.valid) return fail(FDR_E_STATE, "%s: the context holds no re-score rows", who);
    if ((rc = rs_check_k(who, k_in, k_out))) return rc;
    if ((rc = rs_check_queries(who, s.n, q_lo, nq))) return rc;
    if ((rc = rs_check_list_total(who, nq, k_in))) return rc;
    if (nq == 0) return FDR_OK;
    if (!cand_idx || !idx_out || !dist_out) return fail(FDR_E_ARG, "%s: null pointer", who);
    const hipStream_t st = ctx->stream;
    const size_t n_in = (size_t)nq * (size_t)k_in, n_out = (size_t)nq * (size_t)k_out;
    if ((rc = rs_lists_begin(s.lists, st, cand_idx, n_in, n_out))) return rc;
    rs_x2(s.lists, st, s.metric, rs_rows_of(s.csr, s.metric, s.has_values), s.n, q_lo, nq, k_in, k_out);
    return rs_lists_end(s.lists, st, who, s.n, 0, q_lo, k_in, cand_idx, n_out, idx_out, dist_out);
}

// X3 over the work items of the candidate rows (d_indptr, d_cand), which lie on the device
template <int METRIC>
static void rs_x3_launch(RescoreRowSet &s, hipStream_t st, size_t n_items, int64_t q_lo, unsigned rbits,
                         const long long *d_indptr, const int *d_cand) {
    hipLaunchKernelGGL((sparse_rescore_ragged_kernel<METRIC>), dim3((unsigned)n_items), dim3(64), 0, st, (long long)s.n,
                       (long long)q_lo, rbits, rs_rows_of(s.csr, METRIC, s.has_values), (const int2 *)s.items.ptr(),
                       d_indptr, d_cand, s.lists.cnt.ptr(), s.rr.keys.ptr(),
                       reinterpret_cast<unsigned long long *>(s.rr.count.ptr()));
}

// count[r] <- min(count[r], k_top) for the nq rows
__global__ __launch_bounds__(256) void rs_clamp_kernel(long long nq, long long k_top, long long *__restrict__ count) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < nq && count[r] > k_top) count[r] = k_top;
}

// What fdr_rescore_rows_radius and fdr_rescore_rows_refine share once the candidate rows (d_indptr [nq + 1], d_cand,
// `total` > 0 candidates) lie on the device and s.h_items lists their batches; the caller has made `radius` a
// non-negative float in [0, 1] and reserved nothing.  X3; the refusal record into *refused (not ~0: the call is over,
// FDR_OK, nothing written, and the caller words the error); the hit counts, clamped to k_top where k_top > 0; their
// scan into indptr_out; the sort; the split; the result held.
static int rs_ragged_run(RescoreRowSet &s, const RadiusCall &call, float radius, int64_t q_lo, int64_t total,
                         const long long *d_indptr, const int *d_cand, int64_t k_top, u64 *refused) {
    int rc;
    RadiusResult &rr = s.rr;
    const hipStream_t st = call.st;
    const int64_t nq = call.nq;
    const size_t n_items = s.h_items.size();  // (at most total / FDR_MAX_K + nq: below 2^31)
    if ((rc = radius_reserve(rr, call))) return rc;
    if ((rc = s.items.reserve(n_items))) return rc;
    if ((rc = s.lists.cnt.reserve(RS_CNT_WORDS))) return rc;
    if ((rc = rr.keys.reserve((size_t)total))) return rc;
    if ((rc = rr.sorted.reserve((size_t)total))) return rc;
    HIP_TRY(upload(s.items, s.h_items.data(), n_items, st));
    HIP_TRY(hipMemsetAsync(s.lists.cnt.ptr() + RS_CNT_REFUSAL, 0xff, 8, st));
    const unsigned rbits = __builtin_bit_cast(unsigned, radius);
    if (s.metric == FDR_METRIC_JACCARD) rs_x3_launch<FDR_METRIC_JACCARD>(s, st, n_items, q_lo, rbits, d_indptr, d_cand);
    else if (s.metric == FDR_METRIC_WEIGHTED_JACCARD)
        rs_x3_launch<FDR_METRIC_WEIGHTED_JACCARD>(s, st, n_items, q_lo, rbits, d_indptr, d_cand);
    else rs_x3_launch<FDR_METRIC_COSINE>(s, st, n_items, q_lo, rbits, d_indptr, d_cand);
    HIP_TRY(hipGetLastError());
    *refused = ~0ull;
    HIP_TRY(hipMemcpyAsync(refused, s.lists.cnt.ptr() + RS_CNT_REFUSAL, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (*refused != ~0ull) return FDR_OK;  // (nothing has been written to indptr_out)
    if (k_top > 0) {
        hipLaunchKernelGGL(rs_clamp_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, (long long)nq,
                           (long long)k_top, rr.count.ptr());
        HIP_TRY(hipGetLastError());
    }
    rc = radius_offsets(rr, s.tmp, call, "hits", "hit counts", nullptr);
    const long long hits = rr.counted;
    if (rc || hits == 0) return rc;  // (no hit: the empty result is held)
    auto sort = [&](void *tmp, size_t &bytes) {  // (a key lies below 2^62: distance bits <= those of 1.0f)
        return rocprim::segmented_radix_sort_keys(tmp, bytes, rr.keys.ptr(), rr.sorted.ptr(), (unsigned)total, (unsigned)nq,
                                                  d_indptr, d_indptr + 1, 0, 63, st);
    };
    if ((rc = rocprim_run(s.tmp, "rocprim::segmented_radix_sort_keys", sort))) return rc;
    hipLaunchKernelGGL(radius_split_kernel<true>, dim3((unsigned)((hits + 255) / 256)), dim3(256), 0, st, hits,
                       (const u64 *)rr.sorted.ptr(), rr.idx(), reinterpret_cast<float *>(rr.idx() + hits), (long long)nq,
                       (const long long *)rr.off.ptr(), d_indptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    rr.held = hits;
    return FDR_OK;
}

FDR_EXPORT int fdr_rescore_rows_radius(fdr_ctx *ctx, float radius, int64_t q_lo, int64_t nq, const int64_t *cand_indptr,
                                       const int32_t *cand_idx, int64_t *indptr_out) {
    static const char who[] = "rescore_rows_radius";
    int rc = use_device(ctx);
    if (rc) return rc;
    RescoreRowSet &s = ctx->rrs;
    if (!s.valid) return fail(FDR_E_STATE, "%s: the context holds no re-score rows", who);
    RadiusResult &rr = s.rr;
    rr.drop();
    if (!(radius >= 0.0f && radius <= 1.0f))  // (a NaN is not in range)
        return fail(FDR_E_ARG, "%s: the radius must be in [0, 1], got %g", who, (double)radius);
    if (radius == 0.0f) radius = 0.0f;  // (-0 is 0: the kernel compares bit patterns, and -0's lie above every distance's)
    if ((rc = rs_check_queries(who, s.n, q_lo, nq))) return rc;
    if (!cand_indptr || !indptr_out) return fail(FDR_E_ARG, "%s: null indptr pointer", who);
    // ---- cand_indptr, on the host: what keeps the kernel's loads and stores in bounds; the work items with it ----
    if (cand_indptr[0] != 0) return fail(FDR_E_ARG, "%s: cand_indptr starts at %lld, not 0", who, (long long)cand_indptr[0]);
    s.h_items.clear();
    try {  // (the list may reach 2^24 + nq items: no exception leaves the C entry point)
        for (int64_t r = 0; r < nq; ++r) {
            const int64_t len = cand_indptr[r + 1] - cand_indptr[r];
            if (len < 0) return fail(FDR_E_ARG, "%s: query %lld: cand_indptr decreases", who, (long long)(q_lo + r));
            if (cand_indptr[r + 1] > INT32_MAX)
                return fail(FDR_E_ARG, "%s: the rows hold 2^31 candidates or more in all", who);
            for (int64_t b = 0; b * FDR_MAX_K < len; ++b) s.h_items.push_back(make_int2((int)r, (int)b));
        }
    } catch (const std::bad_alloc &) {
        return fail(FDR_E_NOMEM, "%s: out of host memory for the work items", who);
    }
    const int64_t total = cand_indptr[nq];
    if (nq == 0) return radius_none(rr, indptr_out);
    if (total == 0) {  // (no candidate, no hit: the indptr alone)
        for (int64_t r = 0; r <= nq; ++r) indptr_out[r] = 0;
        rr.held = 0;
        return FDR_OK;
    }
    if (!cand_idx) return fail(FDR_E_ARG, "%s: null pointer", who);
    const hipStream_t st = ctx->stream;
    const RadiusCall call = {st, who, nq, INT64_MAX, indptr_out};  // (no cap: the caller supplied the candidates)
    if ((rc = s.cand_indptr.reserve((size_t)nq + 1))) return rc;
    if ((rc = s.lists.cand.reserve((size_t)total))) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "cand_indptr is the sort's segment offsets");
    HIP_TRY(hipMemcpyAsync(s.cand_indptr.ptr(), cand_indptr, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.lists.cand.ptr(), cand_idx, (size_t)total * 4, hipMemcpyHostToDevice, st));
    u64 refused = ~0ull;
    if ((rc = rs_ragged_run(s, call, radius, q_lo, total, s.cand_indptr.ptr(), s.lists.cand.ptr(), 0, &refused))) return rc;
    if (refused != ~0ull) {  // (nothing has been written to indptr_out)
        const long long row = (long long)(refused >> 32), pos = (long long)(refused & 0xffffffffull);
        return fail(FDR_E_ARG, "%s: query %lld, position %lld: the candidate (%d) is no row in [0, %lld)", who,
                    (long long)q_lo + row, pos, cand_idx[cand_indptr[row] + pos], s.n);
    }
    return FDR_OK;
}

// The held expansion (fdr_graph_expand, graph_expand.inc) scored on the held rows, straight from device memory: X3 on
// work items listed from the expansion's host-side row pointer, the hit counts clamped to k_top ahead of the scan, and
// from there fdr_rescore_rows_radius' sort and split unchanged: a row's result is the first min(hits, k_top) keys of
// its sorted segment.  The expansion stays held.
FDR_EXPORT int fdr_rescore_rows_refine(fdr_ctx *ctx, float radius, int32_t k_top, int64_t *indptr_out) {
    static const char who[] = "rescore_rows_refine";
    int rc = use_device(ctx);
    if (rc) return rc;
    RescoreRowSet &s = ctx->rrs;
    if (!s.valid) return fail(FDR_E_STATE, "%s: the context holds no re-score rows", who);
    RadiusResult &rr = s.rr;
    rr.drop();
    const GraphExpandScratch &ge = ctx->ge;
    if (ge.held < 0)
        return fail(FDR_E_STATE, "%s: the context holds no expansion (fdr_graph_expand makes one; the next "
                    "fdr_graph_expand and fdr_graph_free drop it)", who);
    if (k_top < 1) return fail(FDR_E_ARG, "%s: k_top (%d) must be in [1, 2^31)", who, k_top);
    if (!(radius >= 0.0f && radius <= 1.0f))  // (a NaN is not in range)
        return fail(FDR_E_ARG, "%s: the radius must be in [0, 1], got %g", who, (double)radius);
    if (radius == 0.0f) radius = 0.0f;  // (-0 is 0, as in fdr_rescore_rows_radius)
    if (ge.n != s.n)
        return fail(FDR_E_ARG, "%s: the expansion is of a graph on %lld rows, the re-score rows are %lld", who, ge.n, s.n);
    if (!indptr_out) return fail(FDR_E_ARG, "%s: null indptr pointer", who);
    const int64_t nq = ge.nq, total = ge.held;
    if (nq == 0) return radius_none(rr, indptr_out);
    if (total == 0) {  // (no candidate, no hit: the indptr alone)
        for (int64_t r = 0; r <= nq; ++r) indptr_out[r] = 0;
        rr.held = 0;
        return FDR_OK;
    }
    s.h_items.clear();
    try {  // (no exception leaves the C entry point)
        for (int64_t r = 0; r < nq; ++r) {
            const int64_t len = ge.h_off[r + 1] - ge.h_off[r];
            for (int64_t b = 0; b * FDR_MAX_K < len; ++b) s.h_items.push_back(make_int2((int)r, (int)b));
        }
    } catch (const std::bad_alloc &) {
        return fail(FDR_E_NOMEM, "%s: out of host memory for the work items", who);
    }
    const RadiusCall call = {ctx->stream, who, nq, INT64_MAX, indptr_out};  // (no cap: fdr_graph_expand's held)
    u64 refused = ~0ull;
    if ((rc = rs_ragged_run(s, call, radius, ge.q_lo, total, ge.off.ptr(), ge.out.ptr(), k_top, &refused))) return rc;
    if (refused != ~0ull)  // (fdr_graph_expand has checked every index)
        return fail(FDR_E_HIP, "internal: %s: the held expansion names a row outside [0, %lld)", who, s.n);
    return FDR_OK;
}

FDR_EXPORT int fdr_rescore_rows_radius_fetch(fdr_ctx *ctx, int64_t hits, int32_t *idx_out, float *dist_out) {
    static const char who[] = "rescore_rows_radius_fetch";
    if (int rc = use_device(ctx)) return rc;
    if (!ctx->rrs.valid) return fail(FDR_E_STATE, "%s: the context holds no re-score rows", who);
    return radius_fetch(ctx->stream, ctx->rrs.rr, who, rr_next, hits, idx_out, dist_out);
}

