// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit), not compiled on its own.
// ------------------------------------------------------------------------------------------
// S1 .. S4  exact cosine k-NN on sparse feature rows (fdr_knn_sparse), without the projection.
//
// The canonical similarity (DESIGN.md section 4) is the fp32 fma chain over the components in ascending order,
// starting at +0.  A term with a zero factor leaves the accumulator's value unchanged, so the chain over the
// features two rows SHARE, in ascending feature order, is the chain over all components of the densified rows
// (up to the sign of a zero accumulator, which 1 - c cannot see).  The same holds for the norm chain of a row
// over its stored values.  The kernels below therefore give the bits of fdr_knn on the densified matrix:
//   S1 sp_rows_kernel      per row: norm chain over the stored values, rinv, zero flag, xhat = x * rinv; argument
//                          checks (ids in [0, F), strictly ascending; finite values); one posting key per stored
//                          entry whose xhat is not +-0 (an entry with xhat = +-0 cannot change an accumulator)
//   (rocprim radix sort of (feature << 32 | row) keys: the postings, ascending by row inside a feature)
//   S2 sp_postings_kernel  per-feature runs: run offsets (int64), posting rows / values, each entry's run id, and
//                          each run's feature id (runfeat, ascending) with the number of runs (cnt[SP_CNT_RUNS])
//   S3 knn_sparse_kernel   one wave per query: walk the query's features in ascending order; the lanes take the
//                          feature's posting entries and update an LDS hash table keyed by target row that holds the
//                          fp32 accumulator.  A target occurs once per feature, so one lane writes a slot per feature
//                          step and the steps are ordered (no float atomics; the key insert is a compare-and-swap).
//                          Then the keys (dist_bits << 32 | row) with dist < 1 are sorted together with the query's
//                          list, and the list is filled with distance-1 rows in index order (every row outside the
//                          table is at distance exactly 1).  A query whose table would pass SP_LIMIT distinct targets
//                          is handed to ...
//   S3r knn_sparse_kernel<true>  the same over ranges of SP_W consecutive target rows (a range holds at most SP_W
//                          distinct targets, so the table never overflows at any posting length, a feature present
//                          in every row included); each feature's slice of a range is found by binary search in its
//                          ascending posting list, and each range's candidates are merged into the list by
//                          (dist, idx).
//   S4 sp_zero_row_kernel  the closed-form answer of an all-zero query: the first k zero rows (distance 0), then the
//                          first rows that are not zero (distance 1).
// Cost model: the pair updates are sum over features f of df_f^2 (df_f = posting length); each reads an 8-byte
// posting entry (row, value), so the search moves ~8 * sum df_f^2 bytes, mostly from L2.  A range-split query
// costs ceil(n / SP_W) binary searches per stored entry on top.
//
// S1j / S3j / S3rj  exact Jaccard k-NN on the same rows (fdr_knn_sparse_metric, FDR_METRIC_JACCARD).  A row's set is
// its stored entries whose value is not +-0 (every stored entry without values).  With a = |S_q|, b = |S_t|,
// c = |S_q & S_t| and u = a + b - c, dist = (float)((double)(u - c) / (double)u), 0 for u = 0 (DESIGN.md section 4).
//   S1j sp_rows_jaccard_kernel  per row: the argument checks of S1, the set size a_r, the empty flag, one posting key
//                          per present entry; no xhat.  The sort, the run flags, the scan and S2 (without values) follow.
//   S3j / S3rj knn_sparse_kernel<RANGE, FDR_METRIC_JACCARD>  the walk of S3 / S3r with an int32 count in the table
//                          slot: a feature step adds 1 where the cosine instance does its fma (the lanes of a step hit
//                          distinct targets, so a plain LDS increment under the step barrier is enough).  At the end
//                          of a table the sizes a_t of the occupied slots are read and the distance is formed in fp64.
//                          The hand-off at SP_LIMIT, the ranges, the merge, the distance-1 fill and S4 (the empty
//                          rows take the zero rows' place) are shared.
// Cost model: the same sum over features of df_f^2 pair updates, each reading a 4-byte posting entry (the row only).
//
// S1w / S3w / S3rw  exact weighted Jaccard (Ruzicka) k-NN on the same rows (FDR_METRIC_WEIGHTED_JACCARD), values >= 0.
// A row's mass A_r is the fp32 add chain over its stored values in order; the shared weight m(q, t) is the fp32 add
// chain of min(x_qf, x_tf) over the features both rows hold with a value > 0, in ascending order; u = ((double)A_q +
// (double)A_t) - (double)m, dist = (float)((u - m) / u), 0 for u = 0 (DESIGN.md section 4).
//   S1w sp_rows_wjaccard_kernel  per row: the argument checks of S1, a negative value and a mass chain that is not
//                          finite refused too; the mass, the zero flag (mass > 0 ? 0 : 1), one posting key per entry
//                          with a value > 0; the raw value goes where S1 puts xhat, so the sort and S2 follow as for
//                          cosine and pval holds the raw values.
//   S3w / S3rw knn_sparse_kernel<RANGE, FDR_METRIC_WEIGHTED_JACCARD>  the walk of S3 / S3r with the same fp32
//                          accumulator in the table slot: a feature step does acc + min(qv, pval[e]) where the cosine
//                          instance does its fma.  At the end of a table the masses of the occupied slots are read
//                          and the distance is formed in fp64.  Everything else is shared.
// Cost model: that of the cosine search (an 8-byte posting entry per pair update).
//
// The index and its searches.  S1 (S1j), the sort and S2 are the BUILD (fdr_sparse_index_build): what they leave in
// ctx->sp (struct SparseIndex, fedrann_hip.hip: one typed array per buffer) -- the rows (indptr, each stored entry's
// run id efeat, xhat (weighted Jaccard: the raw values), the set sizes asize or the masses mass), the postings (runptr,
// posting_rows(), pval) and the zero flags (zero) -- is the context's one sparse index, described by sp.built; the
// build's scratch (keys, sorted_keys, sorted_pos, tmp) is kept with it.  Two arrays change their contents on the way and
// a third is cut up: the accessors run_flags() / run_numbers(), posting_rows() and zidx() / zdist() of the struct hold
// the casts and say why the first contents are dead by then.  release() frees the arrays and forgets the index in one
// place (fdr_sparse_index_free).  S4, S3 and S3r are a SEARCH (fdr_sparse_index_search) of
// the query rows [q_lo, q_hi) against all n rows: S3's grid is the range, the heavy list and its counter are reset per
// search, and row q - q_lo of the result buffers (sized by the range) is query q.  fdr_knn_sparse[_metric] is a build
// and a search of [0, n) through the same two functions.
//
// The query side.  S3 / S3r read the TARGETS through the postings (runptr, posting_rows(), pval), the targets' set sizes
// or masses and S4's closed-form row, and the QUERIES through one small struct of pointers (SpQuerySide: indptr, efeat,
// xhat, asize, mass, zero, the heavy list) and the first row's number.  A search of the index's own rows passes the
// index's arrays.  fdr_sparse_index_query passes the arrays of a query set that need not be in the index (ctx->spq,
// struct SparseQuerySet: uploaded per call, grown as needed, released with the index), after
//   S1q sp_query_rows_kernel<METRIC>  one thread per query row: the argument checks of S1 / S1j / S1w, the row's rinv /
//                          xhat, set size or mass and its zero flag -- through sp_row<METRIC>, the one device function
//                          the build's S1 kernels call too, so a row gives the same bits on either side -- and for
//                          each stored entry the run of its feature in the index by binary search in runfeat: -1
//                          where no index row holds the feature or where a build would give the entry no posting.
// A query feature without a run counts in the query's norm, size or mass and in nothing else.  S4 runs when a QUERY is
// zero (the index need not hold a zero row), and the zero queries are counted by S1q.  The kernel is the same code
// for both: the heavy list holds row numbers of the query side and has room for all of its rows, and the result row
// is q - q0 with q0 = 0 for a query set.  A refused query (the checks of S1q included) has written nothing of the
// index but the search's counters.
// ------------------------------------------------------------------------------------------
#define SP_CAP 1024    // hash-table slots per query (key int32 | fp32 accumulator or int32 count: 8 KiB of LDS)
#define SP_LOG2CAP 10
#define SP_LIMIT 512   // more distinct targets than this before a chunk of 64 postings: the range-split kernel
#define SP_W 512       // target rows per range of the range-split kernel (<= SP_CAP: the table cannot fill)
#define SP_LIST 128    // the query's list (FDR_MAX_K keys) ahead of the table in the same LDS array
#define SP_EMPTY (-1)
static_assert(SP_LIST >= FDR_MAX_K, "the list holds k keys");
static_assert(SP_LIST + SP_LIMIT + 64 <= SP_LIST + SP_CAP && SP_LIST + SP_W <= SP_LIST + SP_CAP,
              "list + candidates of one range fit the sort buffer");
static_assert((1 << SP_LOG2CAP) == SP_CAP, "SP_CAP is a power of two");

// counters (u64 each): [0, 3) and SP_CNT_RUNS of a build, [3, 6) of a search or a query call
#define SP_CNT_ERR 0      // or of SP_ERR_* bits
#define SP_CNT_DROPPED 1  // stored entries without a posting (xhat = +-0; Jaccard: value = +-0; weighted: not > 0)
#define SP_CNT_ZERO 2     // zero rows (Jaccard: empty rows; weighted Jaccard: zero-mass rows)
#define SP_CNT_HEAVY 3    // queries handed to the range-split kernel
#define SP_CNT_ZEROQ 4    // zero (empty) rows among the queries
#define SP_CNT_QERR 5     // or of SP_ERR_* bits of the query rows (fdr_sparse_index_query)
#define SP_CNT_RUNS 6     // the index's runs (features with a posting): written by S2, kept with the index
#define SP_ERR_RANGE 1u
#define SP_ERR_ORDER 2u
#define SP_ERR_VALUE 4u
#define SP_ERR_NEGATIVE 8u  // weighted Jaccard: a value below 0
#define SP_ERR_MASS 16u     // weighted Jaccard: a row's mass chain is not finite

__device__ __forceinline__ long long sp_lower_bound(const int *__restrict__ a, long long lo, long long hi, int v) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// What S1 / S1j / S1w and the query rows' S1q learn of one row
struct SpRow {
    unsigned err;  // SP_ERR_* bits
    u64 dropped;   // stored entries without a posting
    bool zero;     // the zero rule: norm chain not > 0 (cosine), empty set (Jaccard), mass not > 0 (weighted Jaccard)
    int a;         // |S_r| (Jaccard)
    float mass;    // A_r (weighted Jaccard)
};

// The row arithmetic, once: the argument checks (ids in [0, F), strictly ascending; finite values; weighted Jaccard:
// no negative value, a finite mass), the norm chain over the stored values in order with rinv (cosine), the set size
// over the values that are not +-0 (Jaccard), the mass chain in stored order (weighted Jaccard), and the zero rule.
// entry(j, f, x, keep) is called per stored entry j in stored order: f its feature, x what the postings take of it
// (cosine: xhat = v * rinv; otherwise the raw value), keep whether a build gives it a posting (cosine: x not +-0;
// Jaccard: v not +-0; weighted Jaccard: v > 0; never once the row has shown an error).  An index row (the build) and
// a query row (fdr_sparse_index_query) go through this one function, so a row gives the same bits as either.
template <int METRIC, class Entry>
__device__ __forceinline__ SpRow sp_row(long long F, const int *__restrict__ indices, const float *__restrict__ vals,
                                        long long b, long long e, Entry entry) {
    constexpr bool JAC = METRIC == FDR_METRIC_JACCARD;
    constexpr bool WJ = METRIC == FDR_METRIC_WEIGHTED_JACCARD;
    SpRow r = {0u, 0ull, false, 0, 0.0f};
    float ri = 0.0f;
    if (!JAC && !WJ) {
        float nn = 0.0f;  // the canonical norm chain over the stored values in order (zeros between them add nothing)
        for (long long j = b; j < e; ++j) {
            const float v = vals ? vals[j] : 1.0f;
            nn = __builtin_fmaf(v, v, nn);
        }
        if (nn > 0.0f) ri = (float)(1.0 / sqrt((double)nn));
        r.zero = !(nn > 0.0f);
    }
    long long prev = -1;
    float A = 0.0f;  // the canonical mass chain over the stored values in order (a stored +-0 adds nothing)
    for (long long j = b; j < e; ++j) {
        const long long f = indices[j];
        const float v = vals ? vals[j] : 1.0f;
        if (f < 0 || f >= F) r.err |= SP_ERR_RANGE;
        else if (f <= prev) r.err |= SP_ERR_ORDER;
        prev = f;
        if (!isfinite(v)) r.err |= SP_ERR_VALUE;
        else if (WJ && v < 0.0f) r.err |= SP_ERR_NEGATIVE;
        float x = v;
        bool keep;
        if (JAC) {
            keep = v != 0.0f;  // |S_r|: the stored entries whose value is not +-0
            r.a += keep ? 1 : 0;
        } else if (WJ) {
            A = A + v;
            keep = v > 0.0f;
        } else {
            x = v * ri;
            keep = x != 0.0f;  // (an entry with xhat = +-0 cannot change an accumulator)
        }
        keep = keep && r.err == 0u;
        entry(j, f, x, keep);
        r.dropped += keep ? 0 : 1;
    }
    if (JAC) r.zero = r.a == 0;
    if (WJ) {
        if (!isfinite(A)) r.err |= SP_ERR_MASS;  // (+inf from finite values: the union of a pair would be infinite)
        r.mass = A;
        r.zero = !(A > 0.0f);
    }
    return r;
}

// S1 / S1j / S1w: one thread per row.  xhat: cosine, weighted Jaccard (the raw values); asize: Jaccard; mass:
// weighted Jaccard; the others null
template <int METRIC>
__device__ __forceinline__ void sp_build_row(long long n, long long F, const long long *__restrict__ indptr,
                                             const int *__restrict__ indices, const float *__restrict__ vals,
                                             float *__restrict__ xhat, int *__restrict__ asize,
                                             float *__restrict__ mass, u64 *__restrict__ keys,
                                             unsigned *__restrict__ pos, int *__restrict__ efeat,
                                             unsigned char *__restrict__ zero, u64 *__restrict__ cnt) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const SpRow r = sp_row<METRIC>(F, indices, vals, indptr[q], indptr[q + 1],
                                   [&](long long j, long long f, float x, bool keep) {
                                       if (METRIC != FDR_METRIC_JACCARD) xhat[j] = x;
                                       // (F << 32: after every posting)
                                       keys[j] = keep ? (((u64)f << 32) | (u64)q) : ((u64)F << 32);
                                       pos[j] = (unsigned)j;
                                       efeat[j] = -1;
                                   });
    if (METRIC == FDR_METRIC_JACCARD) asize[q] = r.a;
    if (METRIC == FDR_METRIC_WEIGHTED_JACCARD) mass[q] = r.mass;
    zero[q] = r.zero ? 1 : 0;
    if (r.zero) atomicAdd(&cnt[SP_CNT_ZERO], 1ull);
    if (r.err) atomicOr(&cnt[SP_CNT_ERR], (u64)r.err);
    if (r.dropped) atomicAdd(&cnt[SP_CNT_DROPPED], r.dropped);
}

__global__ __launch_bounds__(256) void sp_rows_kernel(long long n, long long F, const long long *__restrict__ indptr,
                                                      const int *__restrict__ indices, const float *__restrict__ vals,
                                                      float *__restrict__ xhat, u64 *__restrict__ keys,
                                                      unsigned *__restrict__ pos, int *__restrict__ efeat,
                                                      unsigned char *__restrict__ zero, u64 *__restrict__ cnt) {
    sp_build_row<FDR_METRIC_COSINE>(n, F, indptr, indices, vals, xhat, nullptr, nullptr, keys, pos, efeat, zero, cnt);
}

__global__ __launch_bounds__(256) void sp_rows_jaccard_kernel(long long n, long long F,
                                                              const long long *__restrict__ indptr,
                                                              const int *__restrict__ indices,
                                                              const float *__restrict__ vals, int *__restrict__ asize,
                                                              u64 *__restrict__ keys, unsigned *__restrict__ pos,
                                                              int *__restrict__ efeat, unsigned char *__restrict__ zero,
                                                              u64 *__restrict__ cnt) {
    sp_build_row<FDR_METRIC_JACCARD>(n, F, indptr, indices, vals, nullptr, asize, nullptr, keys, pos, efeat, zero, cnt);
}

__global__ __launch_bounds__(256) void sp_rows_wjaccard_kernel(long long n, long long F,
                                                               const long long *__restrict__ indptr,
                                                               const int *__restrict__ indices,
                                                               const float *__restrict__ vals, float *__restrict__ xraw,
                                                               float *__restrict__ mass, u64 *__restrict__ keys,
                                                               unsigned *__restrict__ pos, int *__restrict__ efeat,
                                                               unsigned char *__restrict__ zero,
                                                               u64 *__restrict__ cnt) {
    sp_build_row<FDR_METRIC_WEIGHTED_JACCARD>(n, F, indptr, indices, vals, xraw, nullptr, mass, keys, pos, efeat, zero,
                                              cnt);
}

// S1q: one thread per query row of fdr_sparse_index_query.  The row's own quantities as the build forms an index
// row's (sp_row), and for each stored entry the run of its feature in the index, found by binary search in the runs'
// ascending feature ids (runfeat [runs], runs = cnt[SP_CNT_RUNS] of the build): -1 where the index has no run for
// the feature or where a build would give the entry no posting.  Errors go to cnt[SP_CNT_QERR], the zero (empty)
// queries are counted in cnt[SP_CNT_ZEROQ].
template <int METRIC>
__global__ __launch_bounds__(256) void sp_query_rows_kernel(long long nq, long long F,
                                                            const long long *__restrict__ indptr,
                                                            const int *__restrict__ indices,
                                                            const float *__restrict__ vals, float *__restrict__ xhat,
                                                            int *__restrict__ asize, float *__restrict__ mass,
                                                            int *__restrict__ efeat, unsigned char *__restrict__ zero,
                                                            const int *__restrict__ runfeat, u64 *__restrict__ cnt) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const long long runs = (long long)cnt[SP_CNT_RUNS];
    const SpRow r = sp_row<METRIC>(F, indices, vals, indptr[q], indptr[q + 1],
                                   [&](long long j, long long f, float x, bool keep) {
                                       if (METRIC != FDR_METRIC_JACCARD) xhat[j] = x;
                                       int c = -1;
                                       if (keep) {  // (keep: f in [0, F))
                                           const long long at = sp_lower_bound(runfeat, 0, runs, (int)f);
                                           if (at < runs && runfeat[at] == (int)f) c = (int)at;
                                       }
                                       efeat[j] = c;
                                   });
    if (METRIC == FDR_METRIC_JACCARD) asize[q] = r.a;
    if (METRIC == FDR_METRIC_WEIGHTED_JACCARD) mass[q] = r.mass;
    zero[q] = r.zero ? 1 : 0;
    if (r.zero) atomicAdd(&cnt[SP_CNT_ZEROQ], 1ull);
    if (r.err) atomicOr(&cnt[SP_CNT_QERR], (u64)r.err);
}

__global__ __launch_bounds__(256) void sp_run_flags_kernel(long long m, const u64 *__restrict__ keys,
                                                           int *__restrict__ flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < m) flag[i] = (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1 : 0;
}

// S2: sorted postings -> run offsets, rows, values, and each stored entry's run id (features renumbered densely in
// ascending order, so no array is as long as F); xhat = pval = null (Jaccard): no values; weighted Jaccard: xhat
// holds the raw values.  runfeat[c] = the feature of run c (ascending), *nruns = the number of runs: what a query
// row that is not in the index finds its entries' runs by
__global__ __launch_bounds__(256) void sp_postings_kernel(long long m, const u64 *__restrict__ keys,
                                                          const unsigned *__restrict__ pos,
                                                          const int *__restrict__ run_incl,
                                                          const float *__restrict__ xhat, int *__restrict__ efeat,
                                                          int *__restrict__ prow, float *__restrict__ pval,
                                                          long long *__restrict__ runptr, int *__restrict__ runfeat,
                                                          u64 *__restrict__ nruns) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int c = run_incl[i] - 1;
    const unsigned p = pos[i];
    efeat[p] = c;
    prow[i] = (int)(unsigned)keys[i];
    if (pval) pval[i] = xhat[p];
    if (i == 0 || run_incl[i - 1] != run_incl[i]) {
        runptr[c] = i;
        runfeat[c] = (int)(keys[i] >> 32);
    }
    if (i == m - 1) {
        runptr[c + 1] = m;
        *nruns = (u64)(c + 1);
    }
}

// S4: one wave, sixteen rows per lane and turn; stops once it has k of each kind
__global__ __launch_bounds__(64) void sp_zero_row_kernel(long long n, const unsigned char *__restrict__ zero, int k,
                                                         int *__restrict__ zidx, float *__restrict__ zdist) {
    __shared__ int zr[FDR_MAX_K], nr[FDR_MAX_K];
    const int lane = threadIdx.x;
    int nz = 0, nv = 0;  // zero / non-zero rows found so far (wave-uniform)
    for (long long base = 0; base < n && (nz < k || nv < k); base += 64 * 16) {
        unsigned zm = 0, vm = 0;
        for (int b = 0; b < 16; ++b) {
            const long long r = base + lane * 16 + b;
            if (r < n) {
                if (zero[r]) zm |= 1u << b;
                else vm |= 1u << b;
            }
        }
        int iz = __popc(zm), iv = __popc(vm);
        for (int off = 1; off < 64; off <<= 1) {
            const int a = __shfl_up(iz, off), c = __shfl_up(iv, off);
            if (lane >= off) {
                iz += a;
                iv += c;
            }
        }
        int sz = nz + iz - __popc(zm), sv = nv + iv - __popc(vm);
        for (int b = 0; b < 16; ++b) {
            const int r = (int)(base + lane * 16 + b);
            if ((zm >> b) & 1u) {
                if (sz < k) zr[sz] = r;
                ++sz;
            }
            if ((vm >> b) & 1u) {
                if (sv < k) nr[sv] = r;
                ++sv;
            }
        }
        nz += __shfl(iz, 63);
        nv += __shfl(iv, 63);
    }
    __syncthreads();
    const int zk = min(nz, k);
    for (int i = lane; i < k; i += 64) {  // (n >= k: nv >= k - zk)
        zidx[i] = i < zk ? zr[i] : nr[i - zk];
        zdist[i] = i < zk ? 0.0f : 1.0f;
    }
}

// the zero (empty) rows among the queries [q_lo, q_hi), added to cnt[SP_CNT_ZEROQ]: sixteen rows per thread, one
// atomic per wave that found any
__global__ __launch_bounds__(256) void sp_count_zero_kernel(long long q_lo, long long q_hi,
                                                            const unsigned char *__restrict__ zero,
                                                            u64 *__restrict__ cnt) {
    const long long base = q_lo + ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
    int c = 0;
    for (int b = 0; b < 16; ++b)
        if (base + b < q_hi) c += zero[base + b] != 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0 && c > 0) atomicAdd(&cnt[SP_CNT_ZEROQ], (u64)c);
}

// the slot of target row t (inserted if new); the caller keeps the distinct keys below SP_CAP, so a free slot exists
__device__ __forceinline__ int sp_insert(int *tab, int t, bool &isnew) {
    unsigned s = ((unsigned)t * 0x9E3779B1u) >> (32 - SP_LOG2CAP);
    for (int probe = 0; probe < SP_CAP; ++probe) {
        const int cur = __hip_atomic_load(&tab[2 * s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (cur == t) return (int)s;
        if (cur == SP_EMPTY) {
            const int old = atomicCAS(&tab[2 * s], SP_EMPTY, t);
            if (old == SP_EMPTY) {
                isnew = true;
                return (int)s;
            }
            if (old == t) return (int)s;
        }
        s = (s + 1) & (SP_CAP - 1);
    }
    return -1;  // (unreachable: fewer than SP_CAP distinct keys)
}

// The query side of a search: the rows the queries are taken from.  A search of the index's own rows passes the
// index's arrays (SparseIndex), fdr_sparse_index_query those of the uploaded query set (SparseQuerySet), whose efeat
// S1q has filled with runs of the index.  Rows are numbered as in these arrays; heavy holds such numbers and has room
// for every query of the call.
struct SpQuerySide {
    const long long *indptr;    // [rows + 1]
    const int *efeat;           // each stored entry's run in the index (-1: none)
    const float *xhat;          // cosine: normalised values; weighted Jaccard: raw values; Jaccard: null
    const int *asize;           // Jaccard: the set sizes
    const float *mass;          // weighted Jaccard: the masses
    const unsigned char *zero;  // the zero (empty, zero-mass) flags
    int *heavy;                 // the queries handed to S3r
};

// The table walk of S3 / S3r, shared by the k-NN kernel and the radius kernels (knn_sparse_radius.inc), so a pair gets
// the same accumulator bits on either path: reset the table, then take the query's stored entries [qb, qe) sixty-four
// at a time and their features in ascending order; the lanes take a feature's posting entries (RANGE: its slice of the
// target rows [lo, hi), by binary search) and update the slot of each target.  Returns true where the table would pass
// SP_LIMIT distinct targets before a chunk of 64 postings (never with RANGE): the hand-off to the range form.  One
// wave; ends behind a barrier, the table complete.
template <bool RANGE, int METRIC>
__device__ __forceinline__ bool sp_walk(u64 *__restrict__ tabw, const long long *__restrict__ runptr,
                                        const int *__restrict__ prow, const float *__restrict__ pval,
                                        const int *__restrict__ efeat, const float *__restrict__ xhat, long long qb,
                                        long long qe, int lo, int hi, int lane) {
    constexpr bool JAC = METRIC == FDR_METRIC_JACCARD;
    constexpr bool WJ = METRIC == FDR_METRIC_WEIGHTED_JACCARD;
    int *tab = reinterpret_cast<int *>(tabw);  // slot s: tab[2 s] = target row (SP_EMPTY), tab[2 s + 1] = acc
    for (int i = lane; i < SP_CAP; i += 64) tabw[i] = 0x00000000FFFFFFFFull;  // key SP_EMPTY, acc +0 / count 0
    __syncthreads();
    int count = 0;  // distinct targets in the table (wave-uniform)
    bool overflow = false;
    for (long long j0 = qb; j0 < qe && !overflow; j0 += 64) {
        // lane l holds the query's stored entry j0 + l: its value and its feature's posting slice
        const long long j = j0 + lane;
        int c = -1;
        float qv = 0.0f;
        long long ps = 0, pe = 0;
        if (j < qe) {
            c = efeat[j];
            if (c >= 0) {
                if (!JAC) qv = xhat[j];
                ps = runptr[c];
                pe = runptr[c + 1];
                if (RANGE) {
                    ps = sp_lower_bound(prow, ps, pe, lo);
                    pe = sp_lower_bound(prow, ps, pe, hi);
                }
            }
        }
        u64 live = __ballot(c >= 0 && pe > ps);
        while (live) {  // the features in ascending order (wave-uniform)
            const int src = __builtin_ctzll(live);
            live &= live - 1;
            const float v = __shfl(qv, src);
            const long long s0 = __shfl(ps, src), s1 = __shfl(pe, src);
            for (long long base = s0; base < s1; base += 64) {
                if (!RANGE && count > SP_LIMIT) {
                    overflow = true;
                    break;
                }
                const long long e = base + lane;
                bool isnew = false;
                if (e < s1) {
                    const int s = sp_insert(tab, prow[e], isnew);
                    if (s >= 0) {
                        if (JAC) {
                            tab[2 * s + 1] += 1;  // (a new slot holds 0; one lane per target in a step)
                        } else if (WJ) {
                            float *a = reinterpret_cast<float *>(&tab[2 * s + 1]);
                            *a = (isnew ? 0.0f : *a) + fminf(v, pval[e]);
                        } else {
                            float *a = reinterpret_cast<float *>(&tab[2 * s + 1]);
                            *a = __builtin_fmaf(v, pval[e], isnew ? 0.0f : *a);
                        }
                    }
                }
                count += __popcll(__ballot(isnew));
                __syncthreads();  // (one wave: orders this step's table writes before the next step's reads)
            }
            if (overflow) break;
        }
    }
    return overflow;
}

// The distance of the query from the target t of an occupied table slot w (target | accumulator << 32): qa = |S_q|
// (Jaccard), qm = A_q (weighted Jaccard).  Shared like sp_walk.
template <int METRIC>
__device__ __forceinline__ float sp_slot_dist(u64 w, int t, int qa, double qm, const int *__restrict__ t_asize,
                                              const float *__restrict__ t_mass) {
    if (METRIC == FDR_METRIC_JACCARD) {  // c >= 1 shared features: u = a + b - c >= 1, one fp64 division, one rounding
        const int c = (int)(unsigned)(w >> 32);
        const int u = qa + t_asize[t] - c;
        return (float)((double)(u - c) / (double)u);
    } else if (METRIC == FDR_METRIC_WEIGHTED_JACCARD) {  // m <= min(A_q, A_t) on the bits and both > 0: u >= max(A_q, A_t) > 0
        const double m = (double)__uint_as_float((unsigned)(w >> 32));
        const double u = (qm + (double)t_mass[t]) - m;
        return (float)((u - m) / u);
    }
    return dist_from_sim(__uint_as_float((unsigned)(w >> 32)));
}

// buf[0, P) ascending, P a power of two >= 64: the bitonic network of one wave; ends behind a barrier
__device__ __forceinline__ void sp_bitonic(u64 *buf, int P, int lane) {
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int jj = k2 >> 1; jj > 0; jj >>= 1) {
            for (int p = lane; p < P / 2; p += 64) {
                const int i = ((p & ~(jj - 1)) << 1) | (p & (jj - 1)), ixj = i + jj;
                const u64 a = buf[i], b = buf[ixj];
                if ((a > b) == ((i & k2) == 0)) {
                    buf[i] = b;
                    buf[ixj] = a;
                }
            }
            __syncthreads();
        }
}

// S3 / S3r (METRIC = FDR_METRIC_COSINE), S3j / S3rj (FDR_METRIC_JACCARD: xhat = pval = null, asize = the set sizes)
// and S3w / S3rw (FDR_METRIC_WEIGHTED_JACCARD: xhat / pval = the raw values, mass = the rows' masses): one wave (one
// workgroup) per query; the queries are the rows q0 + blockIdx.x of the query side (S3) or the heavy list's (S3r), and
// query q writes row q - q0 of idx_out / dist_out.  The target side (runptr, prow, pval, t_asize, t_mass, zidx / zdist)
// is the index's
template <bool RANGE, int METRIC>
__global__ __launch_bounds__(64) void knn_sparse_kernel(long long n, long long q0, const SpQuerySide qs,
                                                        const long long *__restrict__ runptr,
                                                        const int *__restrict__ prow, const float *__restrict__ pval,
                                                        const int *__restrict__ t_asize,
                                                        const float *__restrict__ t_mass, int k,
                                                        const int *__restrict__ zidx, const float *__restrict__ zdist,
                                                        u64 *__restrict__ cnt, int *__restrict__ idx_out,
                                                        float *__restrict__ dist_out) {
    const long long *__restrict__ indptr = qs.indptr;
    const int *__restrict__ efeat = qs.efeat;
    const float *__restrict__ xhat = qs.xhat;
    int *__restrict__ heavy = qs.heavy;
    __shared__ u64 buf[SP_LIST + SP_CAP];  // [0, k): the query's list; [SP_LIST, ...): the table, then the sort buffer
    constexpr bool JAC = METRIC == FDR_METRIC_JACCARD;  // (... or the int32 count of shared features: no values)
    constexpr bool WJ = METRIC == FDR_METRIC_WEIGHTED_JACCARD;  // (acc = the fp32 chain of the minima)
    const int lane = threadIdx.x;
    const long long q = RANGE ? (long long)heavy[blockIdx.x] : q0 + (long long)blockIdx.x;
    int *out_i = idx_out + (q - q0) * k;
    float *out_d = dist_out + (q - q0) * k;
    if (!RANGE && qs.zero[q]) {
        for (int i = lane; i < k; i += 64) {
            out_i[i] = zidx[i];
            out_d[i] = zdist[i];
        }
        return;
    }
    const long long qb = indptr[q], qe = indptr[q + 1];
    const int qa = JAC ? qs.asize[q] : 0;  // |S_q|
    const double qm = WJ ? (double)qs.mass[q] : 0.0;  // A_q
    for (int i = lane; i < SP_LIST; i += 64) buf[i] = KEY_INF;
    const long long nranges = RANGE ? (n + SP_W - 1) / SP_W : 1;
    const u64 lt = (1ull << lane) - 1ull;
    for (long long r = 0; r < nranges; ++r) {
        const int lo = RANGE ? (int)(r * SP_W) : 0;
        const int hi = RANGE ? (int)min(n, (long long)lo + SP_W) : (int)n;
        const bool overflow =
            sp_walk<RANGE, METRIC>(buf + SP_LIST, runptr, prow, pval, efeat, xhat, qb, qe, lo, hi, lane);
        if (overflow) {
            if (lane == 0) heavy[atomicAdd(&cnt[SP_CNT_HEAVY], 1ull)] = (int)q;
            return;
        }
        // the table's keys with dist < 1, appended to the list, sorted by (dist, idx)
        u64 cand[SP_CAP / 64];
#pragma unroll
        for (int i = 0; i < SP_CAP / 64; ++i) {
            const u64 w = buf[SP_LIST + lane + 64 * i];
            const int t = (int)(unsigned)w;
            u64 key = KEY_INF;
            if (t != SP_EMPTY) {
                const float d = sp_slot_dist<METRIC>(w, t, qa, qm, t_asize, t_mass);
                if (d < 1.0f) key = ((u64)__float_as_uint(d) << 32) | (unsigned)t;
            }
            cand[i] = key;
        }
        __syncthreads();
        int m = k;
#pragma unroll
        for (int i = 0; i < SP_CAP / 64; ++i) {
            const bool h = cand[i] != KEY_INF;
            const u64 bal = __ballot(h);
            if (h) buf[m + __popcll(bal & lt)] = cand[i];
            m += __popcll(bal);
        }
        int P = 64;
        while (P < m) P <<= 1;
        for (int i = m + lane; i < P; i += 64) buf[i] = KEY_INF;
        __syncthreads();
        sp_bitonic(buf, P, lane);
    }
    // the list's keys (all at dist < 1), then the smallest rows outside it at distance 1
    int have = 0;
    for (int i0 = 0; i0 < k; i0 += 64) have += __popcll(__ballot(i0 + lane < k && buf[i0 + lane] != KEY_INF));
    for (int i = lane; i < have; i += 64) {
        const u64 key = buf[i];
        out_i[i] = (int)(unsigned)key;
        out_d[i] = __uint_as_float((unsigned)(key >> 32));
    }
    int filled = have;
    for (long long base = 0; filled < k; base += 64) {  // (n >= k: ends)
        const long long rr = base + lane;
        bool take = rr < n;
        for (int i = 0; i < have && take; ++i) take = (unsigned)buf[i] != (unsigned)rr;
        const u64 bal = __ballot(take);
        const int at = filled + __popcll(bal & lt);
        if (take && at < k) {
            out_i[at] = (int)rr;
            out_d[at] = 1.0f;
        }
        filled += __popcll(bal);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// S3 over the queries [q_lo, q_lo + nq) of the query side, then S3r over the queries it handed on; h = their number,
// and the zero (empty) rows among the queries.  d_idx / d_dist: [nq, k] results on the device.
template <int METRIC>
static int sp_search(fdr_ctx *ctx, const SpQuerySide &qs, int64_t n, int32_t k, int64_t q_lo, int64_t nq, int *d_idx,
                     float *d_dist, u64 (&h)[2]) {
    const hipStream_t st = ctx->stream;
    SparseIndex &sp = ctx->sp;
    constexpr bool JAC = METRIC == FDR_METRIC_JACCARD;
    constexpr bool WJ = METRIC == FDR_METRIC_WEIGHTED_JACCARD;
    static_assert(SP_CNT_ZEROQ == SP_CNT_HEAVY + 1, "one read-back for both");
    auto launch = [&](auto range, unsigned grid) {  // S3 (std::false_type) or S3r (std::true_type)
        hipLaunchKernelGGL((knn_sparse_kernel<decltype(range)::value, METRIC>), dim3(grid), dim3(64), 0, st, (long long)n,
                           (long long)q_lo, qs, sp.runptr.ptr(), sp.posting_rows(), JAC ? nullptr : sp.pval.ptr(),
                           JAC ? sp.asize.ptr() : nullptr, WJ ? sp.mass.ptr() : nullptr, (int)k, sp.zidx(), sp.zdist(),
                           sp.cnt.ptr(), d_idx, d_dist);
    };
    launch(std::false_type{}, (unsigned)nq);
    HIP_TRY(hipGetLastError());
    h[0] = h[1] = 0;
    HIP_TRY(hipMemcpyAsync(h, sp.cnt.ptr() + SP_CNT_HEAVY, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h[0] > 0) {
        launch(std::true_type{}, (unsigned)h[0]);
        HIP_TRY(hipGetLastError());
    }
    return FDR_OK;
}

// What the row kernels (S1 / S1j / S1w, S1q) found wrong with the rows: FDR_E_ARG and its message, or FDR_OK
static int sp_refuse(const char *who, u64 err, int64_t n_features) {
    if (err & SP_ERR_RANGE) return fail(FDR_E_ARG, "%s: a feature index is outside [0, %lld)", who, (long long)n_features);
    if (err & SP_ERR_ORDER) return fail(FDR_E_ARG, "%s: feature indices must be strictly ascending inside a row", who);
    if (err & SP_ERR_VALUE) return fail(FDR_E_ARG, "%s: non-finite value", who);
    if (err & SP_ERR_NEGATIVE)
        return fail(FDR_E_ARG, "%s: negative value (the weighted Jaccard metric takes values >= 0)", who);
    if (err & SP_ERR_MASS)
        return fail(FDR_E_ARG, "%s: a row's fp32 sum of values is not finite (the weighted Jaccard metric needs a "
                    "finite mass per row)", who);
    return FDR_OK;
}

// The build: the argument checks, the upload, S1 (S1j), the sort, the run flags and scan, S2.  sp.built describes the
// index once everything is enqueued; a refused or failed build leaves none.  `who` names the entry point in messages.
static int sp_build(fdr_ctx *ctx, const char *who, int32_t metric, int64_t n, int64_t n_features, const int64_t *indptr,
                    const int32_t *indices, const float *values) {
    int rc;
    ctx->sp.built = {};
    const bool jac = metric == FDR_METRIC_JACCARD, wj = metric == FDR_METRIC_WEIGHTED_JACCARD;
    if (!jac && !wj && metric != FDR_METRIC_COSINE)
        return fail(FDR_E_ARG, "%s: unknown metric %d (FDR_METRIC_COSINE, FDR_METRIC_JACCARD, "
                    "FDR_METRIC_WEIGHTED_JACCARD)", who, metric);
    if (!indptr) return fail(FDR_E_ARG, "%s: null pointer", who);
    if (n < 1) return fail(FDR_E_ARG, "%s: need at least one row, got n = %lld", who, (long long)n);
    if (n > INT32_MAX) return fail(FDR_E_ARG, "%s: n (%lld) must be below 2^31 rows", who, (long long)n);
    if (n_features < 1 || n_features > INT32_MAX)
        return fail(FDR_E_ARG, "%s: n_features (%lld) must be in [1, 2^31)", who, (long long)n_features);
    if (indptr[0] != 0) return fail(FDR_E_ARG, "%s: indptr[0] must be 0", who);
    for (int64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(FDR_E_ARG, "%s: indptr not monotone at row %lld", who, (long long)i);
    const int64_t nnz = indptr[n];
    if (nnz > INT32_MAX) return fail(FDR_E_ARG, "%s: %lld stored entries (at most 2^31 - 1)", who, (long long)nnz);
    if (nnz > 0 && !indices) return fail(FDR_E_ARG, "%s: indices is null", who);
    const hipStream_t st = ctx->stream;
    SparseIndex &sp = ctx->sp;
    const size_t m1 = (size_t)std::max<int64_t>(nnz, 1);
    if ((rc = sp.indptr.reserve((size_t)(n + 1)))) return rc;
    if ((rc = sp.indices.reserve(m1))) return rc;
    if (values && (rc = sp.values.reserve(m1))) return rc;
    if (!jac && (rc = sp.xhat.reserve(m1))) return rc;
    if (jac && (rc = sp.asize.reserve((size_t)n))) return rc;
    if (wj && (rc = sp.mass.reserve((size_t)n))) return rc;
    if ((rc = sp.keys.reserve(m1))) return rc;
    if ((rc = sp.sorted_keys.reserve(m1))) return rc;
    if ((rc = sp.pos.reserve(m1))) return rc;
    if ((rc = sp.sorted_pos.reserve(m1))) return rc;
    if ((rc = sp.efeat.reserve(m1))) return rc;
    if (!jac && (rc = sp.pval.reserve(m1))) return rc;
    if ((rc = sp.runptr.reserve(m1 + 1))) return rc;
    if ((rc = sp.runfeat.reserve(std::min(m1, (size_t)n_features)))) return rc;  // (a run per feature with a posting)
    if ((rc = sp.heavy.reserve((size_t)n))) return rc;
    if ((rc = sp.cnt.reserve(SparseIndex::cnt_words))) return rc;
    if ((rc = sp.zero.reserve((size_t)n))) return rc;
    u64 *cnt = sp.cnt.ptr();
    HIP_TRY(hipMemcpyAsync(sp.indptr.ptr(), indptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        HIP_TRY(hipMemcpyAsync(sp.indices.ptr(), indices, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        if (values) HIP_TRY(hipMemcpyAsync(sp.values.ptr(), values, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemsetAsync(cnt, 0, 64, st));
    if (jac) {
        hipLaunchKernelGGL(sp_rows_jaccard_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n,
                           (long long)n_features, sp.indptr.ptr(), sp.indices.ptr(), values ? sp.values.ptr() : nullptr,
                           sp.asize.ptr(), sp.keys.ptr(), sp.pos.ptr(), sp.efeat.ptr(), sp.zero.ptr(), cnt);
    } else if (wj) {
        hipLaunchKernelGGL(sp_rows_wjaccard_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n,
                           (long long)n_features, sp.indptr.ptr(), sp.indices.ptr(), values ? sp.values.ptr() : nullptr,
                           sp.xhat.ptr(), sp.mass.ptr(), sp.keys.ptr(), sp.pos.ptr(), sp.efeat.ptr(), sp.zero.ptr(), cnt);
    } else {
        hipLaunchKernelGGL(sp_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n,
                           (long long)n_features, sp.indptr.ptr(), sp.indices.ptr(), values ? sp.values.ptr() : nullptr,
                           sp.xhat.ptr(), sp.keys.ptr(), sp.pos.ptr(), sp.efeat.ptr(), sp.zero.ptr(), cnt);
    }
    HIP_TRY(hipGetLastError());
    u64 h_cnt[3];
    HIP_TRY(hipMemcpyAsync(h_cnt, cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = sp_refuse(who, h_cnt[SP_CNT_ERR], n_features))) return rc;
    const long long kept = (long long)nnz - (long long)h_cnt[SP_CNT_DROPPED];
    if (kept > 0) {
        int end_bit = 32;
        while (end_bit < 64 && ((u64)n_features >> (end_bit - 32)) != 0) ++end_bit;  // (the sentinel F << 32 too)
        int *flag = sp.run_flags(), *run_incl = sp.run_numbers(kept);
        auto sort = [&](void *tmp, size_t &bytes) {
            return rocprim::radix_sort_pairs(tmp, bytes, sp.keys.ptr(), sp.sorted_keys.ptr(), sp.pos.ptr(),
                                             sp.sorted_pos.ptr(), (size_t)nnz, 0, end_bit, st);
        };
        auto scan = [&](void *tmp, size_t &bytes) {
            return rocprim::inclusive_scan(tmp, bytes, flag, run_incl, (size_t)kept, rocprim::plus<int>(), st);
        };
        if ((rc = rocprim_reserve(sp.tmp, sort, scan))) return rc;  // (sized for both: the scan never regrows it)
        if ((rc = rocprim_run(sp.tmp, "rocprim::radix_sort_pairs", sort))) return rc;
        const unsigned g = (unsigned)((kept + 255) / 256);
        hipLaunchKernelGGL(sp_run_flags_kernel, dim3(g), dim3(256), 0, st, kept, sp.sorted_keys.ptr(), flag);
        HIP_TRY(hipGetLastError());
        if ((rc = rocprim_run(sp.tmp, "rocprim::inclusive_scan", scan))) return rc;
        hipLaunchKernelGGL(sp_postings_kernel, dim3(g), dim3(256), 0, st, kept, sp.sorted_keys.ptr(),
                           sp.sorted_pos.ptr(), run_incl, jac ? nullptr : sp.xhat.ptr(), sp.efeat.ptr(),
                           sp.posting_rows(), jac ? nullptr : sp.pval.ptr(), sp.runptr.ptr(), sp.runfeat.ptr(),
                           cnt + SP_CNT_RUNS);
        HIP_TRY(hipGetLastError());
    }
    sp.built.valid = true;
    sp.built.metric = metric;
    sp.built.n = n;
    sp.built.n_features = n_features;
    sp.built.kept = kept;
    sp.built.nzero = (long long)h_cnt[SP_CNT_ZERO];
    return FDR_OK;
}

// The tail of every search: S3 / S3r by the index's metric over the queries [q0, q0 + nq) of the query side (the
// caller has reset the search's counters and enqueued S4 where a query is zero), the results and the trace
static int sp_search_tail(fdr_ctx *ctx, const SpQuerySide &qs, int32_t k, int64_t q0, int64_t nq, int32_t *idx_out,
                          float *dist_out) {
    int rc;
    const hipStream_t st = ctx->stream;
    SparseIndex &sp = ctx->sp;
    const int64_t n = sp.built.n;
    u64 h[2] = {0, 0};  // queries that took S3r; zero (empty) rows among the queries
    if (nq > 0) {
        ResultStaging &res = ctx->res;
        if ((rc = res.idx.reserve((size_t)nq * k))) return rc;
        if ((rc = res.dist.reserve((size_t)nq * k))) return rc;
        int *d_idx = res.idx.ptr();
        float *d_dist = res.dist.ptr();
        if (sp.built.metric == FDR_METRIC_JACCARD)
            rc = sp_search<FDR_METRIC_JACCARD>(ctx, qs, n, k, q0, nq, d_idx, d_dist, h);
        else if (sp.built.metric == FDR_METRIC_WEIGHTED_JACCARD)
            rc = sp_search<FDR_METRIC_WEIGHTED_JACCARD>(ctx, qs, n, k, q0, nq, d_idx, d_dist, h);
        else
            rc = sp_search<FDR_METRIC_COSINE>(ctx, qs, n, k, q0, nq, d_idx, d_dist, h);
        if (rc) return rc;
        HIP_TRY(download(idx_out, res.idx, (size_t)nq * k, st));
        HIP_TRY(download(dist_out, res.dist, (size_t)nq * k, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    fdr_knn_trace &t = ctx->last.trace;
    t.kind = FDR_TRACE_SPARSE;
    t.k = k;
    t.queries = nq;
    t.targets = n;
    t.zero_queries = (int32_t)std::min<u64>(h[1], INT32_MAX);
    t.range_queries = (int32_t)h[0];
    t.range_chunks = h[0] ? (int32_t)((n + SP_W - 1) / SP_W) : 0;
    return FDR_OK;
}

static int sp_zero_row(fdr_ctx *ctx, int32_t k) {  // S4 (depends on k: per search)
    SparseIndex &sp = ctx->sp;
    hipLaunchKernelGGL(sp_zero_row_kernel, dim3(1), dim3(64), 0, ctx->stream, (long long)sp.built.n, sp.zero.ptr(), (int)k,
                       sp.zidx(), sp.zdist());
    HIP_TRY(hipGetLastError());
    return FDR_OK;
}

// A search of the context's index (the caller has checked that there is one, and k and the range): S4 when the index
// has a zero row, S3 / S3r over the queries [q_lo, q_hi), the results and the trace.  The query side is the index itself.
static int sp_search_range(fdr_ctx *ctx, int32_t k, int64_t q_lo, int64_t q_hi, int32_t *idx_out, float *dist_out) {
    int rc;
    const hipStream_t st = ctx->stream;
    SparseIndex &sp = ctx->sp;
    const int64_t nq = q_hi - q_lo;
    if (nq > 0) {
        HIP_TRY(hipMemsetAsync(sp.cnt.ptr() + SP_CNT_HEAVY, 0, 16, st));  // (the heavy list's counter and the zero queries')
        if (sp.built.nzero > 0) {
            if ((rc = sp_zero_row(ctx, k))) return rc;
            hipLaunchKernelGGL(sp_count_zero_kernel, dim3((unsigned)((nq + 4095) / 4096)), dim3(256), 0, st,
                               (long long)q_lo, (long long)q_hi, sp.zero.ptr(), sp.cnt.ptr());
            HIP_TRY(hipGetLastError());
        }
    }
    const SpQuerySide own = {sp.indptr.ptr(), sp.efeat.ptr(), sp.xhat.ptr(),  sp.asize.ptr(),
                             sp.mass.ptr(),   sp.zero.ptr(),  sp.heavy.ptr()};
    return sp_search_tail(ctx, own, k, q_lo, nq, idx_out, dist_out);
}

// The query rows of fdr_sparse_index_query and fdr_sparse_index_radius_query (`who` names the entry point in messages):
// the checks of the query CSR, its upload into the context's query set, the reset of the search's counters and S1q.
// side = the query set as a query side, zeroq = the zero (empty) rows among the queries.  Nothing of the index is
// written except the search's counters.
static int sp_query_side(fdr_ctx *ctx, const char *who, int64_t nq, const int64_t *indptr, const int32_t *indices,
                         const float *values, SpQuerySide &side, u64 &zeroq) {
    int rc;
    const hipStream_t st = ctx->stream;
    SparseIndex &sp = ctx->sp;
    SparseQuerySet &qset = ctx->spq;
    const int metric = sp.built.metric;
    const bool jac = metric == FDR_METRIC_JACCARD, wj = metric == FDR_METRIC_WEIGHTED_JACCARD;
    if (indptr[0] != 0) return fail(FDR_E_ARG, "%s: indptr[0] must be 0", who);
    for (int64_t i = 0; i < nq; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(FDR_E_ARG, "%s: indptr not monotone at row %lld", who, (long long)i);
    const int64_t nnz = indptr[nq];
    if (nnz > INT32_MAX) return fail(FDR_E_ARG, "%s: %lld stored entries (at most 2^31 - 1)", who, (long long)nnz);
    if (nnz > 0 && !indices) return fail(FDR_E_ARG, "%s: indices is null", who);
    const size_t m1 = (size_t)std::max<int64_t>(nnz, 1);
    if ((rc = qset.indptr.reserve((size_t)(nq + 1)))) return rc;
    if ((rc = qset.indices.reserve(m1))) return rc;
    if (values && (rc = qset.values.reserve(m1))) return rc;
    if (!jac && (rc = qset.xhat.reserve(m1))) return rc;
    if ((rc = qset.efeat.reserve(m1))) return rc;
    if (jac && (rc = qset.asize.reserve((size_t)nq))) return rc;
    if (wj && (rc = qset.mass.reserve((size_t)nq))) return rc;
    if ((rc = qset.zero.reserve((size_t)nq))) return rc;
    if ((rc = qset.heavy.reserve((size_t)nq))) return rc;
    HIP_TRY(hipMemcpyAsync(qset.indptr.ptr(), indptr, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        HIP_TRY(hipMemcpyAsync(qset.indices.ptr(), indices, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        if (values) HIP_TRY(hipMemcpyAsync(qset.values.ptr(), values, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    }
    static_assert(SP_CNT_ZEROQ == SP_CNT_HEAVY + 1 && SP_CNT_QERR == SP_CNT_HEAVY + 2, "one reset for the three");
    HIP_TRY(hipMemsetAsync(sp.cnt.ptr() + SP_CNT_HEAVY, 0, 24, st));
    auto rows = [&](auto m) {  // S1q
        hipLaunchKernelGGL((sp_query_rows_kernel<decltype(m)::value>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st,
                           (long long)nq, (long long)sp.built.n_features, qset.indptr.ptr(), qset.indices.ptr(),
                           values ? qset.values.ptr() : nullptr, jac ? nullptr : qset.xhat.ptr(),
                           jac ? qset.asize.ptr() : nullptr, wj ? qset.mass.ptr() : nullptr, qset.efeat.ptr(),
                           qset.zero.ptr(), sp.runfeat.ptr(), sp.cnt.ptr());
    };
    if (jac) rows(std::integral_constant<int, FDR_METRIC_JACCARD>{});
    else if (wj) rows(std::integral_constant<int, FDR_METRIC_WEIGHTED_JACCARD>{});
    else rows(std::integral_constant<int, FDR_METRIC_COSINE>{});
    HIP_TRY(hipGetLastError());
    u64 h[2] = {0, 0};  // zero (empty) queries; error bits
    HIP_TRY(hipMemcpyAsync(h, sp.cnt.ptr() + SP_CNT_ZEROQ, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = sp_refuse(who, h[1], sp.built.n_features))) return rc;
    side = {qset.indptr.ptr(), qset.efeat.ptr(), qset.xhat.ptr(), qset.asize.ptr(),
            qset.mass.ptr(),   qset.zero.ptr(),  qset.heavy.ptr()};
    zeroq = h[0];
    return FDR_OK;
}

// fdr_sparse_index_query behind its checks of the context, k and the result pointers: the query rows, S4 when a query
// is zero, and the search's tail with the query set as the query side.
static int sp_query(fdr_ctx *ctx, int32_t k, int64_t nq, const int64_t *indptr, const int32_t *indices,
                    const float *values, int32_t *idx_out, float *dist_out) {
    int rc;
    SpQuerySide side = {};
    u64 zeroq = 0;
    if ((rc = sp_query_side(ctx, "sparse_index_query", nq, indptr, indices, values, side, zeroq))) return rc;
    if (zeroq > 0 && (rc = sp_zero_row(ctx, k))) return rc;  // (the index need not hold a zero row for a query to be one)
    return sp_search_tail(ctx, side, k, 0, nq, idx_out, dist_out);
}

static int sp_knn(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features, const int64_t *indptr,
                  const int32_t *indices, const float *values, int32_t k, int32_t *idx_out, float *dist_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    ctx->sp.built = {};  // (the call replaces the context's index, also where it is refused before the build)
    ctx->spr.rr.drop();
    if (metric != FDR_METRIC_JACCARD && metric != FDR_METRIC_WEIGHTED_JACCARD && metric != FDR_METRIC_COSINE)
        return fail(FDR_E_ARG, "knn_sparse: unknown metric %d (FDR_METRIC_COSINE, FDR_METRIC_JACCARD, "
                    "FDR_METRIC_WEIGHTED_JACCARD)", metric);
    if (!indptr || !idx_out || !dist_out) return fail(FDR_E_ARG, "knn_sparse: null pointer");
    if (k < 1 || k > FDR_MAX_K) return fail(FDR_E_ARG, "knn_sparse: k=%d unsupported (1..%d)", k, FDR_MAX_K);
    if (n < k) return fail(FDR_E_ARG, "knn_sparse: need n (%lld) >= k (%d)", (long long)n, k);
    if ((rc = sp_build(ctx, "knn_sparse", metric, n, n_features, indptr, indices, values))) return rc;
    return sp_search_range(ctx, k, 0, n, idx_out, dist_out);
}

FDR_EXPORT int fdr_knn_sparse(fdr_ctx *ctx, int64_t n, int64_t n_features, const int64_t *indptr,
                              const int32_t *indices, const float *values, int32_t k, int32_t *idx_out,
                              float *dist_out) {
    return sp_knn(ctx, FDR_METRIC_COSINE, n, n_features, indptr, indices, values, k, idx_out, dist_out);
}

FDR_EXPORT int fdr_knn_sparse_metric(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features,
                                     const int64_t *indptr, const int32_t *indices, const float *values, int32_t k,
                                     int32_t *idx_out, float *dist_out) {
    return sp_knn(ctx, metric, n, n_features, indptr, indices, values, k, idx_out, dist_out);
}

FDR_EXPORT int fdr_sparse_index_build(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features,
                                      const int64_t *indptr, const int32_t *indices, const float *values) {
    int rc = use_device(ctx);
    if (rc) return rc;
    ctx->spr.rr.drop();
    if ((rc = sp_build(ctx, "sparse_index_build", metric, n, n_features, indptr, indices, values))) return rc;
    ctx->sp.built.valid = false;
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (a failure of the sort or of S2 belongs to this call: no index)
    ctx->sp.built.valid = true;
    return FDR_OK;
}

FDR_EXPORT int fdr_sparse_index_search(fdr_ctx *ctx, int32_t k, int64_t q_lo, int64_t q_hi, int32_t *idx_out,
                                       float *dist_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    ctx->spr.rr.drop();
    if (!ctx->sp.built.valid) return fail(FDR_E_STATE, "sparse_index_search: the context holds no sparse index");
    const int64_t n = ctx->sp.built.n;
    if (k < 1 || k > FDR_MAX_K || k > n)
        return fail(FDR_E_ARG, "sparse_index_search: k=%d unsupported (1..min(%d, n = %lld))", k, FDR_MAX_K, (long long)n);
    if (q_lo < 0 || q_hi < q_lo || q_hi > n)
        return fail(FDR_E_ARG, "sparse_index_search: rows [%lld, %lld) are no range of the %lld rows", (long long)q_lo,
                    (long long)q_hi, (long long)n);
    if (q_hi > q_lo && (!idx_out || !dist_out)) return fail(FDR_E_ARG, "sparse_index_search: null pointer");
    return sp_search_range(ctx, k, q_lo, q_hi, idx_out, dist_out);
}

FDR_EXPORT int fdr_sparse_index_query(fdr_ctx *ctx, int32_t k, int64_t nq, const int64_t *q_indptr,
                                      const int32_t *q_indices, const float *q_values, int32_t *idx_out,
                                      float *dist_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    ctx->spr.rr.drop();
    if (!ctx->sp.built.valid) return fail(FDR_E_STATE, "sparse_index_query: the context holds no sparse index");
    const int64_t n = ctx->sp.built.n;
    if (k < 1 || k > FDR_MAX_K || k > n)
        return fail(FDR_E_ARG, "sparse_index_query: k=%d unsupported (1..min(%d, n = %lld))", k, FDR_MAX_K, (long long)n);
    if (nq < 0 || nq > INT32_MAX)
        return fail(FDR_E_ARG, "sparse_index_query: nq (%lld) must be in [0, 2^31)", (long long)nq);
    if (nq == 0) return sp_search_tail(ctx, SpQuerySide{}, k, 0, 0, idx_out, dist_out);  // (the trace alone)
    if (!q_indptr || !idx_out || !dist_out) return fail(FDR_E_ARG, "sparse_index_query: null pointer");
    return sp_query(ctx, k, nq, q_indptr, q_indices, q_values, idx_out, dist_out);
}

FDR_EXPORT int fdr_sparse_index_info(fdr_ctx *ctx, int32_t *metric, int64_t *n, int64_t *postings, int64_t *zero_rows,
                                     size_t *device_bytes) {
    if (!ctx) return fail(FDR_E_ARG, "null context");
    if (!ctx->sp.built.valid) return fail(FDR_E_STATE, "sparse_index_info: the context holds no sparse index");
    if (metric) *metric = ctx->sp.built.metric;
    if (n) *n = ctx->sp.built.n;
    if (postings) *postings = ctx->sp.built.kept;
    if (zero_rows) *zero_rows = ctx->sp.built.nzero;
    if (device_bytes) {
        // (the query set of fdr_sparse_index_query and the buffers of the radius searches too)
        *device_bytes = ctx->sp.bytes() + ctx->spq.bytes() + ctx->spr.bytes();
    }
    return FDR_OK;
}

FDR_EXPORT int fdr_sparse_index_free(fdr_ctx *ctx) {
    int rc = use_device(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->sp.release();
    ctx->spq.release();
    ctx->spr.release();
    return FDR_OK;
}
