/*
 * fedrann_hip.h -- C-ABI of libfedrann_hip.so, the MI355X (gfx950) implementation of FEDRANN's
 * dimensionality-reduction + k-NN hot path.
 *
 * The reference (jzhang-dev/FEDRANN v0.5.4) has no FFI for this path: the seam is three in-process
 * Python calls in fedrann/__main__.py (run_fedrann_pipeline):
 *     get_precompute_matrix(...)            __main__.py:331-335  -> precompute.py:58-115
 *     get_feature_matrix(...)               __main__.py:339-345  -> feature_extraction.py:216-292
 *     get_neighbors_ava(...)                __main__.py:361-365  -> nearest_neighbors.py:22-55
 * Each entry point below names the reference call it replaces.  The Python host
 * (fedrann_amd/) keeps those three call shapes and binds this header through ctypes; the stub a
 * reference maintainer would add is in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no C++ or torch types; every function returns 0 on success or a negative FDR_E_*
 *     code, and fdr_last_error() returns the message of the calling thread's last failure.
 *   - the caller owns every buffer it passes; the library borrows pointers for the duration of the
 *     call only.  "host" functions take host pointers and synchronise before returning; "_dev"
 *     functions take device pointers (hipMalloc'd or a torch tensor's data_ptr()) plus a
 *     hipStream_t passed as void* and enqueue work on that stream.  fdr_embed_dev and fdr_normalize_dev
 *     return without synchronising; fdr_knn_dev synchronises the stream twice on the common path (it sizes its
 *     follow-up passes from counters it reads back: unique-row counts; uncertified / all-zero / plateau queries; below
 *     2^18 targets a duplicate-row probe, and once more when a plateau's range overflows), so work the caller wants
 *     to overlap with it belongs on another stream.
 *   - one context = one GPU; one context per process is the intended use (one process per GPU).
 *     A context is not re-entrant: one call in flight at a time.
 *   - all arrays are C-contiguous with exactly the element types written here.
 */
#ifndef FEDRANN_HIP_H
#define FEDRANN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDR_OK 0
#define FDR_E_ARG (-1)     /* bad argument (null pointer, size, unsupported d or k, ...) */
#define FDR_E_HIP (-2)     /* a HIP runtime call or kernel launch failed */
#define FDR_E_NOMEM (-4)   /* device or host allocation failed */
#define FDR_E_STATE (-5)   /* call order (e.g. embed before a projection was loaded) */
#define FDR_E_IO (-6)      /* a file could not be opened / mapped */

#define FDR_MAX_K 128      /* neighbours per row (self included); up to 64 on every MFMA pass, 65..128 on the exact MFMA
                              pass from 8192 targets (d <= 1024), else on a generic kernel */
#define FDR_MAX_DIM 2048   /* embedding dimension; up to 512 (reference default: 500) on every MFMA pass, up to 1024 on
                              the exact MFMA pass from 8192 targets, beyond on a generic vector-ALU kernel (same results,
                              far slower: DESIGN.md) */

typedef struct fdr_ctx fdr_ctx;

/* ---- lifetime -------------------------------------------------------------------------- */
int fdr_create(int device_id, fdr_ctx **out);
int fdr_destroy(fdr_ctx *ctx);
const char *fdr_last_error(void);
/* "name|gcnArch|CUs|HBM bytes" of the context's device, NUL-terminated into buf. */
int fdr_device_info(fdr_ctx *ctx, char *buf, int buflen);
/* Padded row length (floats) of the internal normalised-embedding layout for dimension d:
 * 128 for d <= 128, 256 for d <= 256, 512 for d <= 512, 1024 for d <= 1024, 2048 for d <= 2048; negative if d is
 * unsupported. */
int fdr_padded_dim(int d);

/* ---- projection (replaces handing `precompute_matrix` to get_feature_matrix,
 *      feature_extraction.py:226-241: P as CSR by feature, float32 data) ---------------------
 * P is n_features x d; p_indptr int64[n_features+1], p_cols int32[nnz] in [0,d), p_vals
 * float32[nnz].  Builds the device-side lookup tables used by the embed kernel. */
int fdr_projection_load(fdr_ctx *ctx, int64_t n_features, int32_t d, const int64_t *p_indptr,
                        const int32_t *p_cols, const float *p_vals);

/* Drop the column ids of a read x feature CSR whose projection row is empty (host only; needs a loaded
 * projection).  P's density is 1/sqrt(F) (precompute.py:80-84): >= 90 % of the features have no entry in P
 * and add nothing to A.dot(P) (feature_extraction.py:204-213), so a caller that compacts its CSR before
 * fdr_embed / fdr_embed_knn moves ~10x fewer bytes over PCIe; E is bit for bit the same (the surviving
 * ids keep their order).  out_indptr int64 [n_rows + 1]; out_indices int32 with room for out_capacity ids
 * (a_indptr[n_rows] always suffices); the outputs must not alias the inputs.  n_threads <= 0: all
 * hardware threads. */
int fdr_csr_compact(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr, const int32_t *a_indices,
                    int64_t *out_indptr, int32_t *out_indices, int64_t out_capacity, int32_t n_threads);

/* Pin / unpin caller-owned host memory (hipHostRegister) so that the host-pointer calls below copy at PCIe
 * rate instead of through a staging buffer.  The caller still owns the memory and must unpin it before
 * freeing it. */
int fdr_host_register(fdr_ctx *ctx, void *ptr, size_t bytes);
int fdr_host_unregister(fdr_ctx *ctx, void *ptr);

/* ---- E = A . P  (replaces process_read_chunk_optimized + the scatter loop,
 *      feature_extraction.py:167-213, :280-290) --------------------------------------------
 * A is the binary read x feature CSR: a_indptr int64[n_rows+1], a_indices int32[nnz], column ids
 * ASCENDING inside each row (scipy canonical form; the host wrapper sorts).  E_out float32
 * [n_rows, d] row-major.  E[r,c] is the sequential fp32 sum, in ascending feature order, of
 * P[f,c] over the features f of row r -- bit-identical to the reference (golden vectors). */
int fdr_embed(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr, const int32_t *a_indices,
              float *E_out);

/* ---- exact cosine k-NN  (replaces NNDescent_ava().get_neighbors(E, metric="cosine",
 *      index_n_neighbors=k, ...).neighbor_graph, nearest_neighbors.py:39-55) ---------------
 * E float32 [n, d] (not normalised).  idx_out int32 [n,k], dist_out float32 [n,k], each row
 * ascending by (distance, index); self is a candidate like any other row.  Canonical arithmetic
 * (DESIGN.md section 4): rows are scaled by (float)(1/sqrt((double)chain(x,x))), the
 * similarity is the fp32 fma chain over components 0..d-1, dist = clamp(1 - c, 0, 1), two
 * all-zero rows are at distance 0.  Requires n >= k, 1 <= k <= FDR_MAX_K, d <= FDR_MAX_DIM (from 8192 targets,
 * 64 < k <= 128 at d <= 512 and any k at 512 < d <= 1024: the exact MFMA pass alone, no prefilter, no duplicate-row
 * classes; d > 1024, or beyond k <= 64, d <= 512 below 8192 targets: the generic kernel, every pair on the vector ALU). */
int fdr_knn(fdr_ctx *ctx, const float *E, int64_t n, int32_t d, int32_t k, int32_t *idx_out,
            float *dist_out);

/* embed + k-NN with E kept in HBM between the two (what run_fedrann_pipeline does in steps 3-4,
 * __main__.py:338-367).  E_out may be NULL. */
int fdr_embed_knn(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr, const int32_t *a_indices,
                  int32_t k, int32_t *idx_out, float *dist_out, float *E_out);

/* ---- exact cosine k-NN on sparse feature rows, without the projection  (replaces
 *      NNDescent_ava().get_neighbors(csr, metric="cosine", index_n_neighbors=k, ...).neighbor_graph for a
 *      csr_matrix argument, nearest_neighbors.py:39-55; pynndescent searches sparse cosine data natively) -----------
 * The rows are a CSR with n rows and n_features columns: indptr int64 [n + 1], indices int32 [indptr[n]] strictly
 * ascending inside each row and in [0, n_features), values float32 [indptr[n]] finite (NULL: every stored entry is
 * 1).  Host pointers; the call synchronises.  idx_out int32 [n, k], dist_out float32 [n, k]: the result of fdr_knn on
 * the densified matrix, bit for bit: the norm chain over a row's stored values in order, the
 * similarity chain over the features two rows share in ascending order, dist = clamp(1 - c, 0, 1), two zero rows at
 * distance 0, (distance, index) order, self a candidate; every row that shares no feature with a non-zero query is
 * at distance exactly 1, so such a list ends in the smallest row indices not already in it.  Limits (FDR_E_ARG):
 * 1 <= k <= FDR_MAX_K, k <= n < 2^31, 1 <= n_features < 2^31, fewer than 2^31 stored entries.  Cost: ~8 bytes per
 * row-pair update, sum over the features of df^2 (df = rows holding the feature); DESIGN.md section 5. */
int fdr_knn_sparse(fdr_ctx *ctx, int64_t n, int64_t n_features, const int64_t *indptr, const int32_t *indices,
                   const float *values, int32_t k, int32_t *idx_out, float *dist_out);

/* ---- the same search under a chosen measure  (NNDescent_ava.get_neighbors(data, metric=...) hands `metric` to
 *      pynndescent, which searches sparse Jaccard natively: nearest_neighbors.py:26, :39-55) -----------------------
 * FDR_METRIC_COSINE is fdr_knn_sparse itself, the same bits.  FDR_METRIC_JACCARD is the exact Jaccard distance of
 * the rows' feature sets.  The set S_r of a row is its stored entries whose value is not +-0
 * (values NULL: every stored entry); non-finite values are refused.  For query q and target t, a = |S_q|, b = |S_t|,
 * c = |S_q & S_t|, u = a + b - c (all below 2^31, exact in a double): dist = 0.0f if u == 0, else
 * (float)((double)(u - c) / (double)u), one IEEE double division and one round-to-nearest conversion: pynndescent's
 * sparse_jaccard value, (union - intersection) / union, stored as float32.  Order (distance bits, index) ascending;
 * self is a candidate at distance 0, an empty row too.  A target that shares no feature with a non-empty query is
 * at exactly 1.0f (as is a pair whose quotient rounds to 1.0f), so a list with fewer than k rows below 1 ends in the
 * smallest row indices not already in it.  An empty query: the first k empty rows at distance 0, then the first
 * non-empty rows at distance 1.  Arguments, limits and error codes are those of fdr_knn_sparse; an unknown metric is
 * FDR_E_ARG.  fdr_last_knn_trace reports FDR_TRACE_SPARSE (zero_queries = the empty rows).  Cost: ~4 bytes per
 * row-pair update (the posting entry is the row alone).
 * FDR_METRIC_WEIGHTED_JACCARD is the exact weighted Jaccard (Ruzicka) distance of rows with values >= 0, 1 - sum of
 * minima / sum of maxima.  A stored +-0 is an absent entry; values NULL: every stored entry is
 * 1.  The mass A_r of a row is the fp32 chain A <- A + x over its stored values in stored order from +0.  The shared
 * weight m(q, t) is the fp32 chain m <- m + min(x_q, x_t) over the features both rows hold with a value > 0, in
 * ascending feature order from +0 (plain fp32 additions, denormals kept).  u = ((double)A_q + (double)A_t) - (double)m
 * in that order: dist = 0.0f if u == 0 (two zero-mass rows), else (float)((u - (double)m) / u), one IEEE double
 * division and one round-to-nearest conversion.  fp32 addition is monotone, so m <= min(A_q, A_t) on the bits and
 * dist lies in [0, 1]; a row is at 0 from itself and its duplicates; with every value 1 and fewer than 2^24 entries
 * per row the result has the bits of FDR_METRIC_JACCARD.  Order (distance bits, index) ascending, self a candidate;
 * rows that share nothing, and pairs whose quotient rounds to 1.0f, are distance-1 rows taken in index order.  A
 * zero-mass query: the first k zero-mass rows at distance 0, then the first other rows at distance 1 (zero_queries
 * counts them).  Refused with FDR_E_ARG, the cause in fdr_last_error: a negative value, a non-finite value, a row
 * whose mass chain is not finite (an overflow to +inf from finite values).  Otherwise arguments, limits and error
 * codes are those of fdr_knn_sparse.  Cost: that of the cosine search, ~8 bytes per row-pair update. */
#define FDR_METRIC_COSINE 0
#define FDR_METRIC_JACCARD 1
#define FDR_METRIC_WEIGHTED_JACCARD 2
int fdr_knn_sparse_metric(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features, const int64_t *indptr,
                          const int32_t *indices, const float *values, int32_t k, int32_t *idx_out, float *dist_out);

/* ---- the sparse search in two steps: build the index once, search row ranges of it  (a host that searches in query
 *      blocks, at several k, or one rank's rows of a row-sharded run: fedrann_amd.distributed.sparse_knn_rank) -------
 * fdr_sparse_index_build does everything of fdr_knn_sparse_metric that does not depend on k or on the queries: the
 * argument checks, the upload of the CSR, the rows' norms (set sizes, masses) and zero flags, the sorted postings.  The index
 * stays in the context, which holds ONE: a build replaces it, and so does every fdr_knn_sparse / fdr_knn_sparse_metric,
 * which is a build followed by a search of [0, n) through the same code (after it, its index is the context's; where
 * it is refused or fails, at any point, the context holds none).  No
 * other call on the context touches the index (fdr_knn, fdr_embed_knn, the _dev calls, the k-mer calls).  Arguments,
 * limits and error codes are those of fdr_knn_sparse_metric, except that there is no k: 1 <= n < 2^31.  A build that
 * is refused (also on the device: an index out of range or out of order, a non-finite value, under
 * FDR_METRIC_WEIGHTED_JACCARD a negative value or a row mass that is not finite; FDR_E_ARG) or that fails
 * leaves NO index, not the earlier one.  Host pointers; the call synchronises. */
int fdr_sparse_index_build(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features, const int64_t *indptr,
                           const int32_t *indices, const float *values);
/* The k nearest rows, among all n rows of the index, of the query rows [q_lo, q_hi): idx_out int32 [q_hi - q_lo, k],
 * dist_out float32 [q_hi - q_lo, k] (host pointers; the call synchronises), row r the query q_lo + r, indices global
 * row numbers: the rows q_lo .. q_hi - 1 of what fdr_knn_sparse_metric gives on the whole CSR, bit for bit, under every
 * rule stated there ((distance bits, index) order, self a candidate, distance-1 rows in index order over all rows, the
 * closed form of a zero or empty query over all rows).  1 <= k <= min(FDR_MAX_K, n) and 0 <= q_lo <= q_hi <= n
 * (FDR_E_ARG); a range shorter than k is fine, q_lo == q_hi is FDR_OK and writes nothing; FDR_E_STATE without an
 * index.  Any number of searches, at any k and over any ranges, follow one build; the device's result buffers are
 * sized by q_hi - q_lo.  fdr_last_knn_trace: FDR_TRACE_SPARSE with queries = q_hi - q_lo, targets = n, and
 * zero_queries / range_queries counting the queries of this call. */
int fdr_sparse_index_search(fdr_ctx *ctx, int32_t k, int64_t q_lo, int64_t q_hi, int32_t *idx_out, float *dist_out);
/* ---- query the index with rows that are not in it  (nearest_neighbors.py:39-55 builds a
 *      pynndescent.NNDescent and reads only its neighbor_graph; this is the shape of that class's
 *      NNDescent.query(query_data, k) -> (indices, distances), exact) ---------------------------------------------------
 * The k nearest rows of the context's index for each of nq query rows, which come as a host CSR of their own: q_indptr
 * int64 [nq + 1] with q_indptr[0] == 0, monotone, fewer than 2^31 stored entries; q_indices int32, in [0, n_features of
 * the index) and strictly ascending inside a row; q_values float32, finite (NULL: every stored entry is 1, whether
 * the index was built with values or not).  idx_out int32 [nq, k] holds row numbers of the index, dist_out float32
 * [nq, k]; host pointers; the call synchronises.  The rules of the index's metric, stated above for fdr_knn_sparse and
 * fdr_knn_sparse_metric, hold unchanged; only the query is no row of the index.  Its own quantities are formed as the
 * build forms a row's, by the same device function: the norm chain over its stored values in order, rinv and xhat =
 * x * rinv (cosine), the set size over the values that are not +-0 (Jaccard), the fp32 mass chain in stored order
 * (weighted Jaccard).  The chain over the shared features runs in ascending feature order (an fma, a +1, or a
 * + min(x_q, x_t) per step), the distance is formed as in a search, the order is (distance bits, index), the distance-1
 * fill runs in index order over all n rows, and a zero, empty or zero-mass QUERY gets the closed form: the first k zero
 * rows of the index at distance 0, then the first other rows at distance 1.  A query feature that no index row holds
 * counts in the query's norm, size or mass and in nothing else.  There is no self: a query equal to an index row
 * finds it at distance 0 like any other row.  So the rows [lo, hi) of the CSR the index was built from, passed as
 * queries with the same values, give fdr_sparse_index_search(k, lo, hi) bit for bit under every metric.
 * 1 <= k <= min(FDR_MAX_K, n); 0 <= nq < 2^31, nq == 0 is FDR_OK and writes nothing; under
 * FDR_METRIC_WEIGHTED_JACCARD values >= 0 and a finite mass chain per row; a null pointer where one is needed, and
 * every violation of the above (the rows' ones found on the device before any search runs): FDR_E_ARG, the cause in
 * fdr_last_error.  FDR_E_STATE without an index.  A refused or failed query leaves the index AS IT WAS (unlike a
 * refused build): a search after it gives the bits from before.  The query rows' device arrays (12 bytes per
 * stored query entry, 8 under Jaccard, and 4 more with values) grow as needed, are counted in fdr_sparse_index_info's device_bytes and are
 * freed by fdr_sparse_index_free; the device's result buffers are sized by nq * k, so a host bounds them by querying in
 * row blocks.  fdr_last_knn_trace: FDR_TRACE_SPARSE with queries = nq, targets = n, zero_queries / range_queries of
 * this call.  Cost: the search's, plus the upload and one binary search over the index's features per stored query
 * entry. */
int fdr_sparse_index_query(fdr_ctx *ctx, int32_t k, int64_t nq, const int64_t *q_indptr, const int32_t *q_indices,
                           const float *q_values, int32_t *idx_out, float *dist_out);
/* ---- radius search: every index row within a distance bound  (scikit-learn's radius_neighbors; the overlapper's
 *      "which reads are within distance r of this one", where a fixed k either cuts a deep region short or pads a
 *      shallow one with distance-1 rows) ----------------------------------------------------------------------------
 * For a query q and a radius r (float32) the result row is every index row t with dist(q, t) <= r.  The comparison is
 * made on the float32 distance a k-NN search of the index reports for that pair, under the index's metric, bit for
 * bit (the same device functions walk the postings and form the distance), and a row is ordered by (distance bits,
 * index) ascending, the k-NN order.  So:
 *   - radius domain: 0 <= r < 1.  NaN, a negative r and r >= 1 are FDR_E_ARG: every row is within 1 of every query, and
 *     ranking them is what fdr_sparse_index_search does;
 *   - a pair at exactly 1.0f is never a hit: a pair without a shared feature, a Jaccard or weighted-Jaccard quotient
 *     that rounds to 1.0f, a cosine similarity <= 0;
 *   - own rows (_radius_search of the rows [q_lo, q_hi)): self is a hit at its distance, as in the k-NN search (the
 *     overlaps writer drops it); outside rows (_radius_query): there is no self;
 *   - a zero, empty or zero-mass query: all zero rows of the index, in index order, at distance 0; none against an
 *     index without zero rows;
 *   - prefix property: for any k, the entries of fdr_sparse_index_search at k with distance <= r are exactly the first
 *     min(k, count) entries of the radius row;
 *   - the index's own rows [lo, hi) passed to _radius_query give _radius_search of [lo, hi) bit for bit.
 * Counts come first.  The call counts every query's hits before it allocates anything for them and writes indptr_out
 * (int64 [queries + 1], a host pointer): indptr_out[0] = 0, the last entry the total, row i's hits at [indptr_out[i],
 * indptr_out[i + 1]).  Only then does it produce the hits, into buffers the context owns (8 bytes per hit held, 8 more
 * of scratch), and fdr_sparse_index_radius_fetch copies them out: idx_out int32 [hits] (rows of the index), dist_out
 * float32 [hits]; its `hits` must equal the total (FDR_E_ARG otherwise).  The pattern of fdr_kmer_search /
 * fdr_kmer_search_indices.  1 <= max_hits < 2^31 (FDR_E_ARG); a total above max_hits is FDR_E_ARG, the message names
 * the total and the cap, and this is the ONE refusal that has written its output: indptr_out is complete and valid,
 * so the caller can cut its row block by the counts.  Nothing was allocated for the hits then, nothing is held for
 * _fetch, and the index is as it was.  The held result is dropped by the next sparse call on the context (a build, a
 * search, a query, a radius call, fdr_sparse_index_free, fdr_knn_sparse[_metric]); _fetch without one is FDR_E_STATE,
 * and a fetch leaves it held.  Without an index the radius calls are FDR_E_STATE.  A refused or failed radius call
 * leaves the index AS IT WAS: a later fdr_sparse_index_search gives the bits from before.  q_lo == q_hi or nq == 0 is
 * FDR_OK with indptr_out[0] = 0.  0 <= q_lo <= q_hi <= n; the query CSR, its checks, limits and messages are those of
 * fdr_sparse_index_query.  Host pointers; the calls synchronise; one GPU (the sharded sparse search has no radius
 * form).  fdr_last_knn_trace: FDR_TRACE_SPARSE with k = 0 and queries, targets, zero_queries, range_queries,
 * range_chunks as for a search.  The buffers (17 bytes per query of the largest call, 16 per hit of the largest
 * result, 4 per zero row) are counted in fdr_sparse_index_info's device_bytes and freed by fdr_sparse_index_free and
 * fdr_destroy.  Cost: the postings are walked twice (count, then emit), about twice the pair updates of a k-NN
 * search of the same queries; DESIGN.md section 5. */
int fdr_sparse_index_radius_search(fdr_ctx *ctx, float radius, int64_t q_lo, int64_t q_hi, int64_t max_hits,
                                   int64_t *indptr_out);
int fdr_sparse_index_radius_query(fdr_ctx *ctx, float radius, int64_t nq, const int64_t *q_indptr,
                                  const int32_t *q_indices, const float *q_values, int64_t max_hits,
                                  int64_t *indptr_out);
int fdr_sparse_index_radius_fetch(fdr_ctx *ctx, int64_t hits, int32_t *idx_out, float *dist_out);
/* The context's index (FDR_E_STATE without one); every out pointer may be NULL.  postings: the stored entries that
 * got a posting (cosine: scaled value not +-0; Jaccard: value not +-0; weighted Jaccard: value > 0).  zero_rows: zero
 * rows (Jaccard: empty rows; weighted Jaccard: zero-mass rows).
 * device_bytes: the device memory the sparse path holds for the context, the build's scratch (unsorted keys, sort
 * buffers) included, which is kept so that the next build allocates nothing, and the query rows of
 * fdr_sparse_index_query: about 52 (cosine, weighted Jaccard) or 44
 * (Jaccard) bytes per stored entry in the library's own buffers, 4 bytes per feature that may get a run (the runs'
 * feature ids, sized by min(stored entries, n_features)), and the radix sort's temporary storage on top, about 12 more
 * per stored entry (64 per stored entry measured at 100 k and 1 M synthetic reads, cosine).  Buffers only grow: after a larger index the figure is the
 * larger one's. */
int fdr_sparse_index_info(fdr_ctx *ctx, int32_t *metric, int64_t *n, int64_t *postings, int64_t *zero_rows,
                          size_t *device_bytes);
/* Drops the index and frees that memory (fdr_destroy does too).  Without an index: FDR_OK. */
int fdr_sparse_index_free(fdr_ctx *ctx);

/* ---- radius search on the projected rows: a dense index held by the context  (the default, embedded path: the same
 *      "which reads are within distance r of this one" as fdr_sparse_index_radius_search, on the rows fdr_embed makes
 *      and fdr_knn searches) -------------------------------------------------------------------------------------------
 * The context holds ONE dense index, beside the sparse one and independent of it.  fdr_dense_index_build takes host
 * rows E float32 [n, d], not normalised (fdr_knn's argument); fdr_dense_index_embed takes fdr_embed's arguments and
 * keeps E in HBM (a projection must be loaded: FDR_E_STATE otherwise).  Either keeps, on the device, the normalised
 * rows in the kernels' layout (fdr_normalize_dev's output, fdr_padded_dim(d) floats per row), the fp16 copy of them
 * that the fp16 passes read, and the zero-row flags.  1 <= n < 2^31; 1 <= d <= 512, the reach of the fp16 passes: a
 * larger d is FDR_E_ARG (there is no vector-ALU or CPU fallback).  A build or embed replaces the index; one that is
 * refused or fails leaves NO index.  No other call on the context touches the index (fdr_knn, fdr_embed_knn, the _dev
 * calls, the sparse and k-mer calls), and the dense-index calls touch neither the sparse index nor fdr_last_knn_trace.
 * Host pointers; the calls synchronise; one GPU.
 * Result contract: that of fdr_sparse_index_radius_search with the canonical dense cosine distance (DESIGN.md section
 * 4) as the metric.  Row i holds every index row t with dist(q_i, t) <= r, the comparison made on the float32 that
 * fdr_knn reports for that pair, ordered by (distance bits, index).  So:
 *   - radius domain: 0 <= r < 1.  NaN, a negative r and r >= 1 are FDR_E_ARG;
 *   - a pair at exactly 1.0f is never a hit (a similarity <= 0; a non-zero query against a zero row);
 *   - own rows (_radius_search of the rows [q_lo, q_hi)): self is a hit at its distance; outside rows (_radius_query,
 *     Q float32 [nq, d] on the host, d the index's): there is no self;
 *   - a zero query: all zero rows of the index, in index order, at distance 0; none against an index without them.  A
 *     non-zero query never hits a zero row;
 *   - prefix property: for any k, the entries of fdr_knn(E, k) with distance <= r are exactly the first min(k, count)
 *     entries of the radius row;
 *   - Q is normalised by the same device function as the index rows, so the rows [lo, hi) of E passed to _radius_query
 *     give _radius_search(lo, hi) bit for bit;
 *   - q_lo == q_hi or nq == 0 is FDR_OK with indptr_out[0] = 0; 0 <= q_lo <= q_hi <= n, 0 <= nq < 2^31.
 * How: an fp16 MFMA range pass over all queries of the call x all rows finds, per query, every row whose approximate
 * distance is within r + 0.001051 (a proven superset of the hits: DESIGN.md section 5), first counting, then emitting;
 * the canonical fp32 chain then decides each candidate.  ONE difference from the sparse call follows: the call must
 * hold the fp16 CANDIDATES before it knows the exact hits, so max_hits (1 <= max_hits < 2^31, FDR_E_ARG otherwise)
 * caps the CANDIDATE total of the call.  A candidate total above max_hits is FDR_E_ARG, and this is the one refusal
 * that has written its output: indptr_out (int64 [queries + 1]) then holds the prefix sums of the per-query candidate
 * counts, which are UPPER BOUNDS of the hit counts (the message says so), and the caller cuts its row block by them.
 * Nothing was allocated for the hits then, nothing is held for _fetch, and the index is as it was.  On success
 * indptr_out is exact: indptr_out[0] = 0, the last entry the total, row i's hits at [indptr_out[i], indptr_out[i + 1]).
 * Device memory for the hits never exceeds 16 bytes x max_hits (8 of keys and 8 of sort space per candidate; the
 * result takes the keys' place), plus 32 bytes of counters per query and the segmented sort's temporary storage.
 * fdr_dense_index_radius_fetch copies the held result out: idx_out int32 [hits] (rows of the index), dist_out float32
 * [hits]; `hits` must equal the total (FDR_E_ARG otherwise); without a held result FDR_E_STATE; a fetch leaves it
 * held, and the next dense-index call (a build, an embed, a radius call, a free) drops it.  Without an index the radius
 * calls are FDR_E_STATE.  A refused or failed radius call leaves the index AS IT WAS.
 * fdr_dense_index_info (FDR_E_STATE without an index; every out pointer may be NULL): n, d; device_bytes, everything
 * the dense index holds on the device, the radius calls' buffers included (buffers only grow: after a larger index
 * or call the figure is the larger one's); of the last radius call its candidates, its hits (candidates >= hits), the
 * query blocks and the target segments of its range pass (0 where it ran none).  fdr_dense_index_free drops the index
 * and frees that memory (fdr_destroy does too); without an index FDR_OK.
 * Limits of the implementation: an index of more than 50 331 648 rows (96 segments of 2^19 rows, what one plan of the
 * fp16 passes holds) is scanned in target chunks of at most that many rows, one launch each; the result is the same.
 * Cost: two fp16 scans of queries x rows plus a tail proportional to the candidates.  The model is about twice the
 * candidate pass of a k-NN search of the same rows; measured, the two scans cost 1.4-2.3 such passes at 100 k rows
 * and 5.1-5.8 at 1 M rows, where the k-NN pass searches unique rows only, skips empty chunks and runs in synchronised
 * rounds and this scan does none of that; DESIGN.md section 5.  Not here: duplicate-row classes, live-chunk skipping,
 * several devices, d > 512. */
int fdr_dense_index_build(fdr_ctx *ctx, const float *E, int64_t n, int32_t d);
int fdr_dense_index_embed(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr, const int32_t *a_indices);
int fdr_dense_index_radius_search(fdr_ctx *ctx, float radius, int64_t q_lo, int64_t q_hi, int64_t max_hits,
                                  int64_t *indptr_out);
int fdr_dense_index_radius_query(fdr_ctx *ctx, float radius, int64_t nq, const float *Q, int64_t max_hits,
                                 int64_t *indptr_out);
int fdr_dense_index_radius_fetch(fdr_ctx *ctx, int64_t hits, int32_t *idx_out, float *dist_out);
int fdr_dense_index_info(fdr_ctx *ctx, int64_t *n, int32_t *d, size_t *device_bytes, int64_t *last_candidates,
                         int64_t *last_hits, int32_t *last_query_blocks, int32_t *last_segments);
int fdr_dense_index_free(fdr_ctx *ctx);

/* ---- merge the candidate lists of a target-sharded sparse search  (fedrann_amd.distributed.sparse_knn_sharded: every
 *      rank indexes its own rows, answers every query among them, and the owner of a query block merges the ranks'
 *      lists) -----------------------------------------------------------------------------------------------------------
 * idx_parts int32 [n_parts, nq, kp] and dist_parts float32 [n_parts, nq, kp], PART-MAJOR: part p's kp candidates of
 * query q at ((p * nq) + q) * kp, the layout a gather by source rank leaves in its receive buffer.  idx_out int32
 * [nq, k], dist_out float32 [nq, k].  Host pointers; the call synchronises.  The key of an entry is
 * (uint64)distance bits << 32 | (uint32)index; row q of the result is the first k entries, ascending by key, of the
 * union of the query's n_parts rows: fedrann_amd.distributed.merge_sparse_topk bit for bit, whose docstring proves
 * that this is the one-GPU search's answer under every sparse rule ((distance bits, index) order, the distance-1 fill in
 * index order, the closed form of a zero query) when each part is a rank's list for the same queries with global indices.
 * Checked on the device before anything is written to idx_out / dist_out (FDR_E_ARG, fdr_last_error names the rule and
 * the smallest (query, part) that breaks one): every index >= 0; every distance a non-negative, non-NaN float (sign
 * bit clear and bits <= 0x7f800000, so bit order is value order); each part's row of each query strictly ascending
 * by key.  NOT checked, the caller's promise: a query's indices are pairwise distinct across its parts; an index that
 * two parts hold at the same distance comes out twice, the lower part's first.  Limits (FDR_E_ARG): 1 <= k <=
 * FDR_MAX_K, 1 <= kp <= FDR_MAX_K, 1 <= n_parts <= 64, n_parts * kp >= k, 0 <= nq < 2^31, nq * kp and nq * k below
 * 2^31; nq == 0 is FDR_OK and writes nothing; a null context, or a null pointer with nq > 0.  The call touches neither
 * the context's sparse index nor fdr_last_knn_trace.  Its device buffers (8 bytes per candidate and per result) belong
 * to the context, only grow and are freed by fdr_destroy.  Cost: the upload of the parts; the kernel reads them once. */
int fdr_topk_merge(fdr_ctx *ctx, int64_t nq, int32_t n_parts, int32_t kp, int32_t k, const int32_t *idx_parts,
                   const float *dist_parts, int32_t *idx_out, float *dist_out);

/* ---- merge the ragged rows of a target-sharded sparse radius search  (fedrann_amd.distributed.sparse_radius_sharded:
 *      every rank indexes its own rows, lists for every query ITS rows within the radius, and the owner of a query block
 *      merges the ranks' rows) ------------------------------------------------------------------------------------------
 * indptr_parts int64 [n_parts, nq + 1], PART-MAJOR, each part's starting at 0: part p holds indptr_parts[p][nq] entries,
 * row q of it at [indptr_parts[p][q], indptr_parts[p][q + 1]).  idx_parts int32 and dist_parts float32: the parts'
 * entries, concatenated in part order (part p's first entry follows part p - 1's last).  indptr_out int64 [nq + 1],
 * idx_out int32 and dist_out float32 [the sum of the parts' totals].  Host pointers; the call synchronises.  The key of
 * an entry is (uint64)distance bits << 32 | (uint32)index; indptr_out[q] is the sum over the parts of indptr_parts[p][q],
 * and row q of the result is the union of the query's n_parts rows, ascending by key:
 * fedrann_amd.distributed.merge_sparse_radius bit for bit, whose docstring argues that this is the one-GPU radius
 * search's row (every target with key <= bound in (distance bits, index) order, a zero query's zero rows at 0 in index
 * order) when each part is a rank's result for the same queries with global indices.
 * Checked on the host before anything is uploaded (FDR_E_ARG): each part's indptr starts at 0 and never decreases; the
 * grand total is below 2^31; 1 <= n_parts <= 64; 0 <= nq < 2^31; a null context, a null indptr pointer, or a null entry
 * pointer with a total > 0.  Checked on the device before anything is written to the out arrays (FDR_E_ARG,
 * fdr_last_error names the rule and the smallest (query, part) that breaks one): every index >= 0; every distance a
 * non-negative, non-NaN float (bits <= 0x7f800000, so bit order is value order); each part's row of each query strictly
 * ascending by key.  On any refusal indptr_out, idx_out and dist_out are untouched.  NOT checked, the caller's promise:
 * a query's indices are pairwise distinct across its parts; a key that two parts hold comes out twice, the lower
 * part's first.  nq == 0 or a total of 0 is FDR_OK with indptr_out written (zeros) and nothing else touched.  The call
 * touches neither the context's sparse index (its held radius result included) nor fdr_last_knn_trace.  Its device
 * buffers (16 bytes per entry, 4 per indptr element, 8 per 64 entries of a query) belong to the context, only grow and are freed by fdr_destroy.
 * Cost: the upload of the parts, plus per entry one binary search in each other part's row of the same query
 * (no sort: the rows are sorted already); DESIGN.md section 5. */
int fdr_radius_merge(fdr_ctx *ctx, int64_t nq, int32_t n_parts, const int64_t *indptr_parts, const int32_t *idx_parts,
                     const float *dist_parts, int64_t *indptr_out, int32_t *idx_out, float *dist_out);

/* ---- symmetrise a neighbour graph: union, mutual and transposed rows  (every search here answers the directed question
 *      "which rows does row q list?", and overlaps.tsv is written from those rows; the reference writes the same directed
 *      pairs, __main__.py get_output_dataframe, and has no counterpart of this call.  An overlap is undirected: its
 *      consumers want row t to name every q that listed t, or only the pairs that list each other, or a row's listers) ----
 * The graph is square, on n rows, as ragged rows: indptr int64 [n + 1], idx int32 and dist float32 [indptr[n]]; an entry
 * (t, d) of row q says "q lists t at distance d", 0 <= t < n.  Rows need not be sorted; a self entry (q, q) is allowed and
 * is its own reverse.  Distances compare by their bit patterns, b(q->t), all at most 0x7f800000.  Row r of the result
 * holds s
 *   FDR_GRAPH_UNION      iff r lists s or s lists r, at the smaller bits of the directions present;
 *   FDR_GRAPH_MUTUAL     iff r lists s and s lists r, at min(b(r->s), b(s->r));
 *   FDR_GRAPH_TRANSPOSE  iff s lists r, at b(s->r);
 * each row strictly ascending by key = (uint64)distance bits << 32 | (uint32)index, as fdr_overlaps_write_csr takes it:
 * fedrann_amd.graph.symmetrize_rows bit for bit, a function of the input alone (two runs give the same bytes).
 * fdr_graph_symmetrize counts: indptr_out int64 [n + 1] takes the result's row pointer, and the entries stay on the device
 * until the next fdr_graph_symmetrize or fdr_graph_free; fdr_graph_symmetrize_fetch copies them out, idx_out int32 and
 * dist_out float32 [entries], entries == indptr_out[n] (another value, or nothing held: an error; 0 entries need no
 * pointers).  Host pointers; both calls synchronise.
 * Checked on the host before anything is uploaded (FDR_E_ARG): the mode; 1 <= n < 2^31; 1 <= max_entries < 2^31; the
 * indptr starts at 0, never decreases and totals below 2^31; null pointers (idx / dist may be null for a graph without
 * entries, whose result is the zero indptr and an empty held result).  Checked on the device before anything is written
 * to indptr_out (FDR_E_ARG, fdr_last_error names the rule and the smallest (row, rule) that breaks one): an index outside
 * [0, n); distance bits above 0x7f800000 (negative, -0.0, NaN); an index listed twice in one row.  A result of more than
 * max_entries entries is refused (FDR_E_ARG) with indptr_out holding the counts, as the radius searches do.  After any
 * refusal nothing is held.
 * The call touches neither the sparse index, the dense index, the re-score rows, their held radius results nor
 * fdr_last_knn_trace.  Its device buffers (32 bytes per input entry, 16 per result entry, 28 per row) belong to the
 * context, only grow and are freed by fdr_graph_free and fdr_destroy.  Cost: two segmented sorts (the input rows by
 * index, the result rows by key) and one binary search per entry in the listed row; DESIGN.md section 5. */
#define FDR_GRAPH_UNION 0
#define FDR_GRAPH_MUTUAL 1
#define FDR_GRAPH_TRANSPOSE 2
int fdr_graph_symmetrize(fdr_ctx *ctx, int32_t mode, int64_t n, const int64_t *indptr, const int32_t *idx,
                         const float *dist, int64_t max_entries, int64_t *indptr_out /* [n + 1] */);
int fdr_graph_symmetrize_fetch(fdr_ctx *ctx, int64_t entries, int32_t *idx_out, float *dist_out);
int fdr_graph_free(fdr_ctx *ctx);

/* ---- connected components of a neighbour graph, cut at a distance  (which reads hang together: bins that assemble
 *      independently, singletons and small islands to drop, the distance at which the graph falls apart.  The reference
 *      has no counterpart: it writes directed pairs, __main__.py get_output_dataframe, and stops) ----
 * The graph is fdr_graph_symmetrize's: n rows, indptr int64 [n + 1], idx int32 and dist float32 [indptr[n]], rows in any
 * order.  For mode FDR_GRAPH_UNION or FDR_GRAPH_MUTUAL and a bound max_distance, rows r != s are joined iff the
 * symmetrised rows of that mode hold the entry (r, s) with distance bits <= bits(max_distance):
 *   FDR_GRAPH_UNION   an entry (q -> t) with bits <= bits(max_distance) joins q and t;
 *   FDR_GRAPH_MUTUAL  q and t are joined iff each lists the other and min(b(q->t), b(t->q)) <= bits(max_distance);
 * a self entry joins nothing; the bound is inclusive and compares bit patterns (0.0 and the smallest subnormal are
 * different distances); +inf joins every entry.  The components are the connected components of those joins.
 * label_out int32 [n]: label_out[r] in [0, C), the components numbered in ascending order of their smallest row, so the
 * labels are a function of the edge set alone (two runs give the same bytes).  size_out int64 [n] or NULL: its first C
 * elements take the components' row counts in label order, the rest are left as they were.  *n_components_out = C.
 * fedrann_amd.graph.component_labels is the model.  Host pointers; the call synchronises.
 * Checked on the host before anything is uploaded (FDR_E_ARG): the mode (FDR_GRAPH_TRANSPOSE is refused: its components
 * are the union's); 1 <= n < 2^31; the bits of max_distance at most 0x7f800000 (NaN, negatives and -0.0 are refused); the
 * indptr starts at 0, never decreases and totals below 2^31; null pointers (idx / dist may be null for a graph without
 * entries, which gives C = n, labels 0 .. n - 1 and sizes of 1 with nothing uploaded).  Checked on the device before
 * anything is written to the outputs (FDR_E_ARG, fdr_last_error names the rule and the smallest (row, rule) that breaks
 * one, in fdr_graph_symmetrize's words, in both modes): an index outside [0, n); distance bits above 0x7f800000; an index
 * listed twice in one row.
 * The call touches neither the sparse index, the dense index, the re-score rows, their held radius results, the held
 * symmetrised graph (fdr_graph_symmetrize_fetch after it still returns that graph) nor fdr_last_knn_trace.  Its device
 * buffers (28 bytes per entry, shared with fdr_graph_symmetrize's input, and 40 per row) belong to the context, only
 * grow and are freed by fdr_graph_free and fdr_destroy.  Cost: one segmented sort (the rows by index), in mutual mode one
 * binary search per entry in the listed row, and a lock-free union-find; DESIGN.md section 5. */
int fdr_graph_components(fdr_ctx *ctx, int32_t mode /* FDR_GRAPH_UNION | FDR_GRAPH_MUTUAL */, int64_t n,
                         const int64_t *indptr, const int32_t *idx, const float *dist, float max_distance,
                         int32_t *label_out /* [n] */, int64_t *size_out /* [n] or NULL */,
                         int64_t *n_components_out);

/* ---- expand a neighbour graph by one hop: the distinct rows within two hops  (the candidate generator of a list
 *      refinement.  The reference's default search is NN-descent, nearest_neighbors.py:39-55, which improves a list by
 *      looking among the neighbours of its neighbours; this call names those, fdr_rescore_rows_refine scores them) ----
 * The graph is fdr_graph_symmetrize's: n rows, indptr int64 [n + 1], idx int32 and dist float32 [indptr[n]], rows in any
 * order.  N_f(x) is the first min(fan, len(x)) entries of row x in ascending order of key = (uint64)distance bits << 32 |
 * (uint32)index.  Row r of the result, for q_lo <= r < q_lo + nq, holds s iff
 *   s is in N_f(r), or
 *   s != r and s is in N_f(t) for some t in N_f(r);
 * each row strictly ascending by index, every index once, at most fan + fan^2 entries: fedrann_amd.graph.expand_rows bit
 * for bit, a function of the input alone (two runs give the same bytes).  A row's own index stays exactly when the row
 * lists itself inside its fan, so whatever convention the search had survives.
 * fdr_graph_expand counts: indptr_out int64 [nq + 1] takes the exact prefix sums, and the indices stay on the device,
 * beside the held symmetrised graph and independent of it, until the next fdr_graph_expand or fdr_graph_free;
 * fdr_graph_expand_fetch copies them out, idx_out int32 [entries], entries == indptr_out[nq] (another value: FDR_E_ARG;
 * nothing held: FDR_E_STATE; 0 entries need no pointer).  Host pointers; both calls synchronise.
 * Checked on the host (FDR_E_ARG): 1 <= fan <= FDR_MAX_K; 1 <= n < 2^31; [q_lo, q_lo + nq) is a range of the rows (nq == 0
 * is FDR_OK and holds an empty result); 1 <= max_entries < 2^31; the indptr starts at 0, never decreases and totals
 * below 2^31; null pointers (idx / dist may be null for a graph without entries); the block's upper bound, the sum over
 * its rows r of |N_f(r)| + the sum over t in N_f(r) of |N_f(t)|, is below 2^31 (it is formed on the device in 64 bits
 * and compared on the host before indptr_out is written; the message says to take fewer rows a call).  Checked on the
 * device before anything is written to indptr_out (FDR_E_ARG, in fdr_graph_symmetrize's words, the smallest (row, rule)
 * named), over the WHOLE graph, because any row can be some t: an index outside [0, n); distance bits above 0x7f800000.
 * NOT refused: an index listed twice in one row.  It takes two places of the fan cut and comes out once.  A result of
 * more than max_entries entries is refused (FDR_E_ARG) with indptr_out holding the counts.  After any refusal nothing
 * is held.
 * The call touches neither the sparse index, the dense index, the re-score rows, their held radius results, the held
 * symmetrised graph nor fdr_last_knn_trace.  Device memory: 24 bytes per input entry (shared with
 * fdr_graph_symmetrize's input), 12 per entry of the upper bound, 4 per result entry, 8 per row of the graph and 24 per
 * row of the block, and rocprim's temporary storage; the buffers belong to the context, only grow and are freed by
 * fdr_graph_free and fdr_destroy.  Cost: one segmented sort of the input rows by key, one of the bound's 32-bit indices
 * by row, two scans; DESIGN.md section 5 (X4). */
int fdr_graph_expand(fdr_ctx *ctx, int64_t n, const int64_t *indptr, const int32_t *idx, const float *dist, int32_t fan,
                     int64_t q_lo, int64_t nq, int64_t max_entries, int64_t *indptr_out /* [nq + 1] */);
int fdr_graph_expand_fetch(fdr_ctx *ctx, int64_t entries, int32_t *idx_out);

/* ---- re-score candidate lists by exact distance on the sparse rows  (the second stage of an approximate search:
 *      NNDescent_ava.get_neighbors on the embeddings names the neighbours, nearest_neighbors.py:39-55, the boundary this
 *      library replaces; their distances there are the projection's, and this call puts the feature rows' own in their
 *      place) ---------------------------------------------------------------------------------------------------------
 * The rows are the CSR of fdr_knn_sparse_metric under its rules: indptr int64 [n + 1], indices int32 strictly ascending
 * inside a row and in [0, n_features), values float32 finite (NULL: every stored entry is 1), under
 * FDR_METRIC_WEIGHTED_JACCARD none negative and a finite mass chain per row; the rows' violations are found on the
 * device before anything is written.  cand_idx int32 [nq, k_in]: row r holds the candidates of query q_lo + r, row
 * numbers in [0, n).  idx_out int32 [nq, k_out], dist_out float32 [nq, k_out]: row r holds that query's candidates
 * under `metric`, ascending by (distance bits, index), the first k_out of them.  Host pointers; the call synchronises.
 * dist(q, t) is, bit for bit, the float32 fdr_knn_sparse_metric on the same CSR reports for the pair whenever t is in
 * q's list (DESIGN.md section 4 for the arithmetic, section 5 for the argument): a row's norm, set size or mass as a
 * build forms it; over the features both rows hold, in ascending feature order from +0, the fp32 fma chain of
 * xhat_q * xhat_t and dist = clamp(1 - c, 0, 1) (cosine), the int32 count c of the features present in both (value not
 * +-0) and (float)((double)(u - c) / (double)u) with u = a + b - c (Jaccard), the fp32 chain m <- m + min(x_q, x_t)
 * and (float)((u - m) / u) with u = ((double)A_q + (double)A_t) - (double)m (weighted Jaccard).  Two zero / empty /
 * zero-mass rows are at 0.0f, exactly one such row at 1.0f, two rows that share nothing at exactly 1.0f.  So the lists
 * of fdr_knn_sparse_metric at k, fed back with k_in = k_out = k, come back unchanged.  The query's own index is an
 * ordinary candidate and comes out at its distance (0).
 * Limits (FDR_E_ARG, the cause in fdr_last_error): 1 <= k_out <= k_in <= FDR_MAX_K; 0 <= q_lo, 0 <= nq, q_lo + nq <= n;
 * 1 <= n < 2^31, 1 <= n_features < 2^31, fewer than 2^31 stored entries, nq * k_in below 2^31; an unknown metric; a null
 * pointer where one is needed.  nq == 0 is FDR_OK and writes nothing.  Checked on the device before anything is written
 * to idx_out / dist_out (FDR_E_ARG, fdr_last_error names the smallest (query, slot)): every candidate in [0, n).  NOT
 * checked, as with fdr_topk_merge: a query's candidates are pairwise distinct; a repeated index comes out twice.
 * The call touches neither the context's sparse index (its held radius result included), nor its dense index, nor
 * fdr_last_knn_trace.  Each call uploads the CSR; its device buffers (4 bytes per stored entry, 4 more with values, 4
 * more under cosine and weighted Jaccard, 1 more under Jaccard with values; 4 per candidate, 8 per result) belong to
 * the context, only grow and are freed by fdr_destroy.  A query row is staged FDR_RESCORE_TILE stored entries at a time;
 * a longer row is walked tile by tile, which changes no bit.  Cost: per pair the candidate's stored entries are read
 * once per tile of the query (4 to 8 bytes each), plus the upload; DESIGN.md section 5. */
#define FDR_RESCORE_TILE 512 /* stored entries of a query row staged at once */
int fdr_sparse_rescore(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features, const int64_t *indptr,
                       const int32_t *indices, const float *values, int64_t q_lo, int64_t nq, int32_t k_in,
                       const int32_t *cand_idx /* [nq, k_in] */, int32_t k_out, int32_t *idx_out,
                       float *dist_out /* [nq, k_out] */);

/* ---- a held row set for re-scoring, rectangular and ragged  (the same boundary, nearest_neighbors.py:39-55: the rows
 *      stay on the device for any number of re-score calls, and a radius result of the projected rows, ragged and of
 *      hundreds of candidates per read, is re-scored and cut by a second bound in the exact metric) ----------------------
 * The context holds ONE re-score row set, beside its sparse index and its dense index and independent of both, and of
 * fdr_sparse_rescore, whose scratch and behaviour are untouched.  Host pointers; the calls synchronise; one GPU.
 * fdr_rescore_rows_build takes the CSR arguments of fdr_sparse_rescore under its rules and limits (1 <= n < 2^31, 1 <=
 * n_features < 2^31, fewer than 2^31 stored entries, a known metric, indptr starting at 0 and never decreasing: FDR_E_ARG
 * otherwise), uploads the CSR once and runs the row pass once; the rows' violations (an id outside [0, n_features) or
 * not strictly ascending inside a row, a value that is not finite, under FDR_METRIC_WEIGHTED_JACCARD a negative value or
 * a mass chain that is not finite) are found on the device and refuse the build (FDR_E_ARG).  A build replaces the
 * previous row set and drops a held radius result; one that is refused or fails leaves NO row set.  Without a row set
 * _info, _knn, _radius and _radius_fetch are FDR_E_STATE, and _free is FDR_OK.  Device memory of the rows: 8 bytes per
 * row for the indptr, 4 per stored entry, 4 more under cosine and weighted Jaccard, 1 more under Jaccard with values,
 * 1 to 5 per row.  Buffers only grow, with two deliberate exceptions, both at a build: the values as given are released
 * once the row pass has read them, and what the new metric does not use of a set built under another metric is released
 * too, so device_bytes never counts dead arrays.  _free and fdr_destroy release everything.  fdr_rescore_rows_info (every out pointer may be NULL): the metric, n, the stored entries,
 * and device_bytes, everything the row set holds on the device, the calls' buffers included.
 * fdr_rescore_rows_knn is fdr_sparse_rescore on the held rows: the same contract, limits and refusals without the CSR
 * arguments (1 <= k_out <= k_in <= FDR_MAX_K; [q_lo, q_lo + nq) a range of the rows; nq * k_in below 2^31; nq == 0 is
 * FDR_OK and writes nothing; every candidate in [0, n), checked on the device before anything is written, the smallest
 * (query, slot) named), and the same bits as fdr_sparse_rescore on the same CSR.  It neither drops nor uses the held
 * radius result.  NOT checked: that a query's candidates are pairwise distinct.
 * fdr_rescore_rows_radius: cand_indptr int64 [nq + 1] and cand_idx int32 [cand_indptr[nq]]; row r of the input is
 * cand_idx[cand_indptr[r] .. cand_indptr[r + 1]), the candidates of query q_lo + r: row numbers in [0, n), of any count,
 * in any order (a row of fdr_dense_index_radius_search, for one).  Row r of the result holds every candidate t of that
 * row with dist(q, t) <= radius, the comparison made on the float32 that fdr_sparse_rescore and fdr_knn_sparse_metric
 * report for the pair (a pair's chain depends on its two rows alone, not on the list it stands in), ordered by
 * (distance bits, index).  indptr_out int64 [nq + 1]: the exact prefix sums, indptr_out[0] = 0.  The result is held and
 * fdr_rescore_rows_radius_fetch copies it out: idx_out int32 [hits], dist_out float32 [hits]; `hits` must equal the
 * total (FDR_E_ARG otherwise); without a held result FDR_E_STATE; a fetch leaves it held, and the next
 * fdr_rescore_rows_* call other than _info, _knn and _radius_fetch drops it (_refine holds its own in its place).  So:
 *   - radius domain: 0 <= radius <= 1.  NaN, a negative radius and one above 1 are FDR_E_ARG; -0.0f is 0;
 *   - radius == 1 keeps every candidate (a distance lies in [0, 1]): the plain ragged re-score, indptr_out = cand_indptr;
 *   - below 1 a pair at exactly 1.0f is no hit, the radius searches' rule;
 *   - the closed forms are fdr_sparse_rescore's: two zero / empty / zero-mass rows at 0.0f, exactly one such row at
 *     1.0f, two rows that share nothing at exactly 1.0f; the query's own index is an ordinary candidate at distance 0;
 *   - nq == 0 (indptr_out[0] = 0) and a total of 0 (every entry 0) are FDR_OK, an empty result held.
 * Checked on the host before any upload (FDR_E_ARG): cand_indptr[0] == 0; cand_indptr never decreases; the total is
 * below 2^31; [q_lo, q_lo + nq) is a range of the rows; no null pointer where one is needed.  Checked on the device
 * before indptr_out is written (FDR_E_ARG): every candidate in [0, n); fdr_last_error names the smallest (query,
 * position in its row) and the value, indptr_out is untouched and no result is held.  NOT checked, the caller's
 * promise: a row's candidates are pairwise distinct; a repeated candidate comes out as often as it goes in.  There is
 * no max_hits: the caller supplies the candidates and so knows the cap on the hits.  Device memory of a call: 16 bytes
 * per candidate (8 of keys, which take the result afterwards; 8 of sort space), 4 more per candidate, 24 per query, 8
 * per FDR_MAX_K candidates of a row, and the segmented sort's temporary storage.  The calls touch neither the sparse
 * index, the dense index, their held results, fdr_sparse_rescore's scratch nor fdr_last_knn_trace.
 * How: a wave scores one batch of at most FDR_MAX_K consecutive candidates of a row, so a row of 5 000 candidates is
 * 40 waves; the keys land in the candidates' places, one segmented sort orders each row, and the hits, the first keys
 * of each sorted row, are compacted.  Cost: per pair the candidate's stored entries are read once per tile of the
 * query, as in fdr_sparse_rescore, without its upload; DESIGN.md section 5 (X3).  Not here: several devices, device
 * pointers.
 * fdr_rescore_rows_refine scores the context's HELD expansion (fdr_graph_expand) on the held rows, straight from device
 * memory: the candidates never pass through host memory.  With the expansion's q_lo, nq and rows, row r of the result is
 * what fdr_rescore_rows_radius(radius, q_lo, nq, the expansion) would hold, cut to its first k_top entries: the same
 * kernel on work items listed from the expansion's host-side row pointer, the hit counts clamped to k_top ahead of their
 * scan, the sort and the split unchanged.  indptr_out int64 [nq + 1]; the result is held and fetched with
 * fdr_rescore_rows_radius_fetch under the rules above; the expansion stays held.  radius == 1 and k_top >= fan + fan^2
 * is the plain ragged re-score of the expansion.  Refused: k_top outside [1, 2^31) and a radius outside [0, 1]
 * (FDR_E_ARG; -0.0f is 0); no row set, or no held expansion (FDR_E_STATE); an expansion of a graph whose n differs from
 * the rows' n (FDR_E_ARG); a null indptr_out.  Device memory and cost: fdr_rescore_rows_radius' without the candidates'
 * upload (16 bytes per candidate of the expansion, 24 per row, 8 per FDR_MAX_K candidates of a row); DESIGN.md section
 * 5 (X4).  Not here: NN-descent's new / old flags, sampling, several devices, device pointers. */
int fdr_rescore_rows_build(fdr_ctx *ctx, int32_t metric, int64_t n, int64_t n_features, const int64_t *indptr,
                           const int32_t *indices, const float *values);
int fdr_rescore_rows_info(fdr_ctx *ctx, int32_t *metric, int64_t *n, int64_t *stored, size_t *device_bytes);
int fdr_rescore_rows_free(fdr_ctx *ctx);
int fdr_rescore_rows_knn(fdr_ctx *ctx, int64_t q_lo, int64_t nq, int32_t k_in, const int32_t *cand_idx /* [nq, k_in] */,
                         int32_t k_out, int32_t *idx_out, float *dist_out /* [nq, k_out] */);
int fdr_rescore_rows_radius(fdr_ctx *ctx, float radius, int64_t q_lo, int64_t nq, const int64_t *cand_indptr /* [nq + 1] */,
                            const int32_t *cand_idx, int64_t *indptr_out /* [nq + 1] */);
int fdr_rescore_rows_radius_fetch(fdr_ctx *ctx, int64_t hits, int32_t *idx_out, float *dist_out);
int fdr_rescore_rows_refine(fdr_ctx *ctx, float radius, int32_t k_top, int64_t *indptr_out /* [nq + 1] */);

/* ---- device-resident API (multi-GPU host, bench.py) ----------------------------------------
 * All pointers are device pointers; work is enqueued on `stream` (a hipStream_t). */
int fdr_embed_dev(fdr_ctx *ctx, int64_t n_rows, const int64_t *d_indptr, const int32_t *d_indices,
                  float *d_E, void *stream);
/* E [n_rows,d] -> Ehat [n_rows, fdr_padded_dim(d)] in the kernel's internal layout (normalised,
 * zero padded, components permuted inside groups of 8) + zero-row flags uint8[n_rows]. */
int fdr_normalize_dev(fdr_ctx *ctx, const float *d_E, int64_t n_rows, int32_t d, float *d_Ehat,
                      uint8_t *d_zero, void *stream);
/* bytes of scratch fdr_knn_dev needs for (nq queries, nt targets, k). */
size_t fdr_knn_workspace_bytes(fdr_ctx *ctx, int64_t nq, int64_t nt, int32_t d, int32_t k);
/* k-NN of nq query rows against nt target rows, both in the Ehat layout.  Neighbour indices are
 * target row numbers + t_base.  Rows of a row-sharded run: queries = the rank's shard, targets =
 * the all-gathered Ehat of every rank.  The result arrays are complete when the call returns AND the
 * stream has finished (see "Conventions": the call itself waits for the stream a few times). */
int fdr_knn_dev(fdr_ctx *ctx, const float *d_Qhat, const uint8_t *d_qzero, int64_t nq,
                const float *d_That, const uint8_t *d_tzero, int64_t nt, int64_t t_base, int32_t d,
                int32_t k, int32_t *d_idx, float *d_dist, void *d_workspace, size_t workspace_bytes,
                void *stream);
/* ---- duplicate-row classes across the ranks of a row-sharded run -----------------------------------
 * fdr_knn_dev searches a duplicate QUERY row once per rank that holds a member of its class.  With these
 * three calls the ranks split the UNIQUE rows instead (same results):
 *   fdr_knn_classes_dev  builds the classes of the target set (the all-gathered Ehat: the same tables on
 *                        every rank) in the workspace -- fdr_knn_workspace_bytes(ctx, nq_max, nt, d, k) bytes,
 *                        nq_max = the most unique rows one later call will search -- and returns their number
 *                        in *n_unique_out; 0 = not worth it (small set, or unique^2 > 0.9 rows^2): use fdr_knn_dev.
 *                        The decision is a function of the exact unique count: the same on every rank.
 *   fdr_knn_unique_dev   k-NN of the unique rows [u_lo, u_hi) (ascending representative order) against all
 *                        unique rows: d_idx_u int32 [u_hi - u_lo, k] (unique-row numbers), d_dist_u float32.
 *   fdr_knn_expand_dev   given the results of ALL unique rows (the ranks' shares concatenated: [n_unique, k]),
 *                        the neighbours of the original rows [q0, q0 + nq): d_idx (+ t_base), d_dist [nq, k].
 *                        u_row_stride = elements between two unique rows' results in d_idx_u_all / d_dist_u_all
 *                        (0 = k; 2 k when a row's indices and distance bits travel side by side in ONE exchange:
 *                        d_dist_u_all = (float *)(d_idx_u_all + k)).
 * The workspace must stay untouched between the three calls; fdr_knn_classes_dev synchronises the stream. */
int fdr_knn_classes_dev(fdr_ctx *ctx, const float *d_That, const uint8_t *d_tzero, int64_t nt, int32_t d, int32_t k,
                        int64_t nq_max, void *d_workspace, size_t workspace_bytes, void *stream,
                        int32_t *n_unique_out);
int fdr_knn_unique_dev(fdr_ctx *ctx, int64_t u_lo, int64_t u_hi, int32_t *d_idx_u, float *d_dist_u, void *stream);
int fdr_knn_expand_dev(fdr_ctx *ctx, int64_t q0, int64_t nq, int64_t t_base, const int32_t *d_idx_u_all,
                       const float *d_dist_u_all, int64_t u_row_stride, int32_t *d_idx, float *d_dist, void *stream);

/* ---- per-kernel timing (bench.py's roofline figures) -----------------------------------------
 * With timing enabled every kernel launch is bracketed by its own hipEvent pair recorded on the
 * stream the kernel is launched on.  fdr_timing_read() waits for the recorded launches of one kernel
 * kind, returns how many there were and their summed duration, and clears the tally. */
#define FDR_KERNEL_EMBED 0
#define FDR_KERNEL_NORMALIZE 1
#define FDR_KERNEL_KNN_TILE 2
#define FDR_KERNEL_KNN_MERGE 3
#define FDR_KERNEL_KNN_PREFILTER 4 /* fp16 MFMA candidate pass of the prefilter mode: one span per launch, or one span
                                      over the whole pass when its launches overlap (fdr_last_prefilter_launches) */
#define FDR_KERNEL_KNN_RERANK 5    /* rest of the prefilter mode: fp16 conversion, key merge, certificate +
                                      exact fp32 re-rank (two timed spans per call) */
#define FDR_KERNEL_KNN_DEDUP 6     /* duplicate-row classes: hash, sort, class tables, gathers, expansion */
#define FDR_KERNEL_KMER_SEARCH 7   /* k-mer search: library table build + the search passes */
#define FDR_KERNEL_KMER_COMPACT 8  /* k-mer search: sort, de-duplication, row pointers */
#define FDR_NUM_KERNELS 9
int fdr_timing(fdr_ctx *ctx, int enable);
int fdr_timing_read(fdr_ctx *ctx, int which, int *count_out, float *total_ms_out);
/* ---- k-NN mode ---------------------------------------------------------------------------------
 * Both modes return the SAME canonical result.  EXACT: every pair through the
 * fp32 MFMA kernel.  PREFILTER (k <= 56): an fp16 MFMA pass proposes k + 12 (or k + 8) candidates per
 * query; a certificate proves they contain the exact top-k and their distances are recomputed with
 * the canonical fp32 chain; queries that cannot be certified are searched by the exact kernel.  The
 * prefilter mode reads one 4-byte counter back per call (a stream synchronisation).  AUTO (default):
 * PREFILTER when it applies and there are >= 8192 targets.  A new context starts in the mode named by
 * the environment variable FDR_KNN_MODE=exact|prefilter|auto (read once, in fdr_create; default auto) --
 * the only environment variable the library reads. */
#define FDR_MODE_AUTO 0
#define FDR_MODE_EXACT 1
#define FDR_MODE_PREFILTER 2
int fdr_set_knn_mode(fdr_ctx *ctx, int mode);
/* Duplicate-row classes: bitwise-identical rows are searched once and the result
 * expanded -- the same canonical result either way.  AUTO (default): from 8192 targets, when at least 5 % of
 * the rows repeat.  OFF: never.  ON: at every size (same 5 % test).  FORCE: always expand, even without
 * duplicates (the parity tests' "+classes" variants). */
#define FDR_DEDUP_AUTO 0
#define FDR_DEDUP_OFF 1
#define FDR_DEDUP_ON 2
#define FDR_DEDUP_FORCE 3
int fdr_set_dedup_mode(fdr_ctx *ctx, int mode);
/* Live-chunk candidate pass: at d <= 128 and K' <= 32 the fp16 pass of a 256-query block skips
 * the 16-component chunks that are empty in every query of the block (knn_prefilter_live_kernel<NL>; blocks with
 * seven or eight live chunks keep the dense kernel) -- the same bits either way.  AUTO (default): where the
 * eight-wave shape runs in synchronised rounds.  OFF: never.  FORCE: at every size, on the eight-wave shape (the
 * parity tests). */
#define FDR_LIVE_AUTO 0
#define FDR_LIVE_OFF 1
#define FDR_LIVE_FORCE 2
int fdr_set_live_chunks(fdr_ctx *ctx, int mode);
/* Stage skipping of the live-chunk pass: a work item visits stage 0 of its segment and the
 * stages -- 128 consecutive rows of the scan order -- that share a chunk with its query block's mask; in every other
 * stage each similarity is exactly 0.  AUTO (default): whenever the live-chunk pass runs.  OFF: every stage, through
 * the same kernels (the parity tests, A/B measurements). */
#define FDR_SKIP_AUTO 0
#define FDR_SKIP_OFF 1
int fdr_set_live_skip(fdr_ctx *ctx, int mode);
/* The end of the live-chunk pass (DESIGN.md sections 5 and 6; docs/experiments.md A-36).  The pass's groups share no
 * bound words and no lists, and a query's candidate lists are complete as soon as its own group's last launch has ended,
 * so neither the order of the groups nor the moment a group's queries are merged and re-ranked changes a result.
 * AUTO (default): the groups in descending cost -- the dense group first, NL = 6 down to the cheapest -- so that the pass
 * drains on its shortest work items.  The second part, the merge + re-rank of every group but the last on a further
 * stream under the pass's final launches, gained less than the run-to-run range and is not part of AUTO.  OFF: ascending
 * NL, and one merge + re-rank of all queries behind the join (the parity tests, A/B measurements).  The other values
 * force a part whatever AUTO makes of it (the parity tests, A/B measurements): ORDER = the descending order alone;
 * EARLY = that + the early work once only the final launch of every queue is outstanding; EARLY_GROUP = that + each
 * group's work right behind the group's own last launch. */
#define FDR_TAIL_AUTO 0
#define FDR_TAIL_OFF 1
#define FDR_TAIL_ORDER 2
#define FDR_TAIL_EARLY 3
#define FDR_TAIL_EARLY_GROUP 4
int fdr_set_pass_tail(fdr_ctx *ctx, int mode);
/* Compact re-rank (DESIGN.md sections 5 and 6): where the padded width is 128 (d <= 128) the prefilter mode keeps, beside the fp16 copies, one
 * fixed-size record per target row that lists the row's non-zero components in the order of the canonical chain, and
 * the certificate kernel re-ranks a candidate from its record; a row with more non-zeros than a record holds takes
 * the dense route (its whole fp32 row) -- the same bits either way.  AUTO (default): the records are built wherever
 * the width allows and read unless more than 1 target row in 32 is too long for its record (then nearly every query
 * would run both routes).  OFF: no records are built and every candidate takes the dense route (the parity tests,
 * A/B measurements).  FORCE: built and read wherever the width allows, however many rows are long (the parity tests). */
#define FDR_COMPACT_AUTO 0
#define FDR_COMPACT_OFF 1
#define FDR_COMPACT_FORCE 2
int fdr_set_rerank_compact(fdr_ctx *ctx, int mode);
/* Diagnostics (test support): the stage lists of target segment `segment` of the most recent call that ran the
 * live-chunk pass.  *first_row_out (may be NULL) = the segment's first row in the scan order, *nstages_out = its stages
 * of 128 rows; lens[256] (may be NULL) = per block mask value the number of
 * stages a block of that mask walks; lists[256][nstages] (may be NULL) = the stage numbers, ascending, 0xffff behind a
 * list's end.  The lists are a copy the context owns, taken while FDR_CAPTURE_LIVE_LISTS is set
 * (fdr_set_knn_capture): FDR_E_STATE when the last k-NN call ran no live-chunk pass or captured none. */
int fdr_last_live_stage_lists(fdr_ctx *ctx, int32_t segment, int32_t *first_row_out, int32_t *nstages_out, int32_t *lens,
                              uint16_t *lists);
/* Unique target / query rows the most recent k-NN call
 * actually searched (= the row counts when the call found too few duplicates to bother). */
int fdr_last_unique(fdr_ctx *ctx, int *unique_targets, int *unique_queries);
/* Prefilter mode only: how the fp16 candidate pass of the most recent k-NN call was launched -- the number
 * of kernel launches and of queues they were dealt to (with two queues two launches are in flight at any
 * time and FDR_KERNEL_KNN_PREFILTER is ONE timed span over the whole pass; 0 / 0 after an exact-mode call). */
int fdr_last_prefilter_launches(fdr_ctx *ctx, int *launches, int *queues);
/* Diagnostics (test support; nothing in the product reads it): which kernels the most recent k-NN call ran.  With
 * the duplicate-row layer active it describes the inner search of the unique rows.  Every k-NN entry point
 * (fdr_knn_dev, fdr_knn, fdr_embed_knn, fdr_knn_classes_dev, fdr_knn_unique_dev, fdr_knn_expand_dev, fdr_knn_sparse,
 * fdr_knn_sparse_metric, fdr_sparse_index_search, fdr_sparse_index_query, fdr_sparse_index_radius_search,
 * fdr_sparse_index_radius_query) clears it, and
 * the per-query path codes, before it checks its arguments. */
#define FDR_TRACE_NONE 0       /* no k-NN search ran (a cleared trace, or a call that failed or found nothing to do) */
#define FDR_TRACE_EXACT 1      /* exact mode: the fp32 kernel for every query */
#define FDR_TRACE_PREFILTER 2  /* fp16 candidate pass + certificate (+ range pass, + exact fallback) */
#define FDR_TRACE_GENERIC 3    /* d > 1024, or k > 64 / d > 512 below 8192 targets: the generic kernel */
#define FDR_TRACE_SPARSE 4     /* fdr_knn_sparse, fdr_sparse_index_search / _query, the radius searches (k = 0):
                                  zero_queries = zero rows among the queries;
                                  range_queries = queries whose targets
                                  overflowed the table and were searched over row ranges, range_chunks = the ranges
                                  of each */
#define FDR_FALLBACK_NONE 0
#define FDR_FALLBACK_CHUNKED 1 /* the uncertified queries gathered and searched by the exact kernel, in chunks */
#define FDR_FALLBACK_WHOLE 2   /* more than half the non-zero queries uncertified: the exact kernel for every query */
typedef struct fdr_knn_trace {
    int32_t kind;              /* FDR_TRACE_* */
    int32_t dp, k, kp;         /* padded dimension, neighbours, candidates per query of the pass (prefilter only) */
    int64_t queries, targets;  /* rows of the search described (the unique rows with the duplicate-row layer) */
    /* candidate pass (prefilter only) */
    int32_t pass_waves;        /* waves per workgroup: 4 or 8 */
    int32_t pass_wps;          /* waves per SIMD of the shape: 4 (128 VGPRs), 3 (168), 2 (256) */
    int32_t pass_units;        /* one-tile stage units of the LDS ring */
    int32_t pass_list_keys;    /* keys per register list: 16 (K' <= 32) or 32 */
    int32_t pass_pingpong;     /* 1: knn_prefilter_pp_kernel */
    int32_t pass_launches, pass_queues, pass_segments;
    /* certificate outcome (read back by the host) and range pass */
    int32_t uncertified, zero_queries;  /* rows sent to the exact list by the certificate; all-zero queries */
    int32_t range_queries;     /* plateau queries of the range pass */
    int32_t range_chunks;      /* its launches (at most 32768 queries each) ... */
    int32_t range_pp_chunks;   /* ... of them on knn_range_pp_kernel (>= 4096 queries in the chunk) */
    int32_t range_w8_chunks;   /* ... of them on the eight-wave d <= 128 range kernel */
    int32_t range_overflow;    /* exact-list entries added by the range pass (sets above its capacity) */
    /* exact fp32 kernel */
    int32_t exact_fallback;    /* FDR_FALLBACK_* (prefilter only) */
    int32_t exact_calls;       /* searches on the exact kernel (whole call = 1; chunked fallback = its chunks) */
    int32_t exact_queries;     /* queries they searched */
    int32_t exact_waves, exact_qsets;  /* shape of the last one: waves per workgroup, query sets per wave (0: none) */
    int32_t generic;           /* 1: the generic kernel ran */
    int32_t exact_segments;    /* target segments of the last exact-kernel search (0: none) */
    /* live-chunk candidate pass (prefilter only) */
    int32_t pass_live;         /* 1: the pass ran grouped by live chunks (knn_prefilter_live_kernel<NL> + the dense kernel) */
    int32_t pass_live_items[5];    /* its work items (query block x segment) on the NL = 2, 3, 4, 5, 6 instances */
    int32_t pass_live_dense_items; /* ... and on the dense kernel (blocks with seven or eight live chunks) */
    int32_t skip_live;             /* 1: its work items walked stage lists that leave disjoint stages out (fdr_set_live_skip) */
    int64_t skip_stages_walked;    /* stages (128 target rows) on the lists of the NL instances' work items (summed by the host) ... */
    int64_t skip_stages_skipped;   /* ... and left out: walked + skipped = the stages of their segments */
    /* compact re-rank (prefilter only; fdr_set_rerank_compact) */
    int64_t rerank_compact_long;    /* target rows with more non-zeros than a record holds (counted by the build) */
    int32_t rerank_compact;         /* 1: knn_rerank_kernel read the records (0: none built, or too many long rows) */
    int32_t rerank_compact_entries; /* non-zeros a record holds (0: no records were built) */
    /* the end of the live-chunk pass (prefilter only; fdr_set_pass_tail) */
    int32_t pass_group_order;       /* its groups in issue order, four bits each from the lowest: NL = 2 .. 6, 8 = the dense group */
    int32_t rerank_early_queries;   /* queries merged and re-ranked under the pass, before the join (0: all behind it) */
} fdr_knn_trace;
int fdr_last_knn_trace(fdr_ctx *ctx, fdr_knn_trace *out);
/* Prefilter mode only: number of query rows of the most recent k-NN call whose candidate set could
 * not be certified and that were therefore searched by the exact kernel. */
int fdr_last_uncertified(fdr_ctx *ctx);
/* Diagnostics: which way each query row of the most recent fdr_knn_dev / fdr_knn / fdr_embed_knn call took to its
 * (canonical, identical on every way) result -- one byte per query row, copied to host memory `paths` [n_queries]:
 * the low seven bits one of FDR_PATH_*, bit 7 (FDR_PATH_CLASS_MEMBER) set when the row belongs to a duplicate-row
 * class of several rows and its result was expanded from the class representative's.  The codes live in the
 * workspace of that call: ask before the workspace is reused or freed, with the n_queries of that call
 * (FDR_E_STATE otherwise, and after fdr_knn_unique_dev / fdr_knn_expand_dev, which record none).  The parity
 * tests stratify their oracle samples by these codes; nothing in the product reads them. */
#define FDR_PATH_NONE 0            /* (never reported for a finished row) */
#define FDR_PATH_CERTIFIED 1       /* fp16 candidates certified, the K' candidates re-ranked with the canonical chain */
#define FDR_PATH_RANGE 2           /* plateau: every target within the bound collected by the range pass, ranked exactly */
#define FDR_PATH_EXACT 3           /* the exact fp32 kernel (exact mode; uncertifiable queries of the prefilter mode) */
#define FDR_PATH_ZERO 4            /* all-zero query row: closed-form answer */
#define FDR_PATH_RANGE_OVERFLOW 5  /* the range pass collected more than its capacity: the exact kernel */
#define FDR_PATH_GENERIC 6         /* d > 1024, or k > 64 / d > 512 below 8192 targets: the generic kernel */
#define FDR_PATH_CLASS_MEMBER 0x80
int fdr_last_query_paths(fdr_ctx *ctx, uint8_t *paths, int64_t n_queries);
/* Diagnostics (test support; nothing in the product reads it): a copy of the prefilter mode's intermediate results,
 * so that the tests can check the fp16 candidate pass and the range pass against a plain model.  `what` or's the
 * FDR_CAPTURE_* flags (default 0: nothing is captured, and the only cost is one host-side branch).  While a flag is
 * set, every prefilter-mode search copies, in stream order, into buffers the context owns (the caller's workspace may
 * be freed as soon as the call returns):
 *   FDR_CAPTURE_CANDIDATES  the merged candidate lists, n_queries x K' keys (fdr_last_candidates);
 *   FDR_CAPTURE_RANGE       per range-pass query: its query row, the bound theta, the count of targets the pass
 *                           found with d~ <= theta and the first min(count, 1024) of them (fdr_last_range_sets).
 *   FDR_CAPTURE_LIVE_LISTS  the live-chunk pass's stage lists, where that pass runs (fdr_last_live_stage_lists).
 * With the duplicate-row layer active the capture describes the inner search of the unique rows.  Every k-NN entry
 * point clears the capture; asking after an exact-mode, generic, failed or non-capturing call is FDR_E_STATE. */
#define FDR_CAPTURE_CANDIDATES 1
#define FDR_CAPTURE_RANGE 2
#define FDR_CAPTURE_LIVE_LISTS 4  /* the live-chunk pass's stage lists (fdr_last_live_stage_lists) */
#define FDR_RANGE_CAP 1024  /* row slots per range query of fdr_last_range_sets */
int fdr_set_knn_capture(fdr_ctx *ctx, int what);
/* The candidate lists of the last call: keys [n_queries, kp] (n_queries and kp = K' as in fdr_last_knn_trace), one
 * ascending list per query.  key = (fp32 bits of d~) << 32 | target row, with d~ = qd / QM1 the approximate
 * distance on the pass's grid of QM1 = 2^qbits - 2 steps and the target row a GLOBAL index (t_base + local row);
 * unused slots are all ones.  *qbits_out (may be null) receives qbits. */
int fdr_last_candidates(fdr_ctx *ctx, uint64_t *keys, int64_t n_queries, int32_t kp, int32_t *qbits_out);
/* The range-pass queries of the last call (n_range = range_queries of fdr_last_knn_trace), in the order the pass took
 * them: queries [n_range] (local query rows), theta [n_range] (the pass admitted d~ <= theta, d~ = 1 - clamp(s~, 0, 1)
 * in fp32), counts [n_range] (targets found: may exceed FDR_RANGE_CAP) and rows [n_range, FDR_RANGE_CAP]: the first
 * min(count, FDR_RANGE_CAP) entries of a query's row are the GLOBAL target rows collected, in no order; the rest -1. */
int fdr_last_range_sets(fdr_ctx *ctx, int64_t n_range, int32_t *queries, float *theta, int32_t *counts, int32_t *rows);

/* ---- k-mer search on the GPU: reads x k-mer library -> per-read set of library indices -----------
 * Replaces the reference's native tool kmer_searcher (kmer_searcher/kmer_searcher.cpp:232-375; called
 * from fedrann/count_kmers.py:131-139).  lib_codes: the unique valid library k-mers in index order as
 * 2-bit codes (A C G T = 0 1 2 3, first base in the most significant position; kmer_to_int :138-151).
 * seqs: the reads' characters concatenated, read r = seqs[seq_off[r] .. seq_off[r+1]).  A character
 * outside ACGTacgt makes every window that contains it invalid in the reference's particular way (see
 * kmer_search.inc).  Output: CSR rows of ascending unique library indices per read (the reference
 * writes them in hash-set order): indptr_out int64 [n_reads + 1] and *nnz_out from fdr_kmer_search,
 * then the indices (int32 [nnz], kept on the device until then) from fdr_kmer_search_indices, which also
 * releases the search's device scratch (~28 B per base: not to be held through the embed / k-NN stages).
 * Limits: the concatenated reads must be shorter than 2^32 characters and, with that scratch, fit in HBM. */
int fdr_kmer_search(fdr_ctx *ctx, const uint8_t *seqs, const int64_t *seq_off, int64_t n_reads,
                    const uint64_t *lib_codes, int64_t n_lib, int32_t k, int64_t *indptr_out,
                    int64_t *nnz_out);
int fdr_kmer_search_indices(fdr_ctx *ctx, int32_t *indices_out);

/* ---- canonical k-mer counting on the GPU ---------------------------------------------------------
 * Replaces `jellyfish count -m k -C` + `jellyfish dump -L min_count` (fedrann/count_kmers.py:80-121):
 * every window of k characters inside one read whose characters are all in ACGTacgt counts once under
 * the smaller of its 2-bit code and its reverse complement's.  fdr_kmer_count keeps the k-mers with at
 * least min_count occurrences on the device and returns their number; fdr_kmer_count_fetch copies
 * them out in ascending code order (jellyfish dumps in its hash order; the order only names the
 * features): codes_out, counts_out uint64 [n], and releases the device scratch.
 * Any number of characters: read sets of 2^31 characters and more are counted in blocks of whole reads whose
 * sorted (code, count) runs are merged into one table on the device; min_count applies to the totals.  Limits:
 * n_reads < 2^31, one read < the block size, < 2^31 distinct k-mers.  fdr_set_kmer_count_block sets the block
 * size in characters (0 = the default 2^31; for tests), fdr_last_kmer_count_blocks returns the number of
 * non-empty blocks the last fdr_kmer_count call counted. */
int fdr_kmer_count(fdr_ctx *ctx, const uint8_t *seqs, const int64_t *seq_off, int64_t n_reads, int32_t k,
                   int64_t min_count, int64_t *n_out);
int fdr_kmer_count_fetch(fdr_ctx *ctx, uint64_t *codes_out, uint64_t *counts_out);
/* The same in pieces, for a reader that streams the reads (the reference pipes them through jellyfish,
 * count_kmers.py:80-99) and never holds the whole read set: begin, add whole reads any number of times (seq_off[0] = 0
 * in every piece), finish = fdr_kmer_count's threshold and result; then fdr_kmer_count_fetch. */
int fdr_kmer_count_begin(fdr_ctx *ctx, int32_t k);
int fdr_kmer_count_add(fdr_ctx *ctx, const uint8_t *seqs, const int64_t *seq_off, int64_t n_reads);
int fdr_kmer_count_finish(fdr_ctx *ctx, int64_t min_count, int64_t *n_out);
int fdr_set_kmer_count_block(fdr_ctx *ctx, int64_t chars);
int fdr_last_kmer_count_blocks(fdr_ctx *ctx);
/* Counting over the ranks of a sharded run: each rank counts its share of the reads (begin / add, no threshold), exports
 * its table cut at n_parts - 1 ascending splitter codes, part p goes to rank p, and each rank merges the runs it received.
 *   fdr_kmer_count_export_dev: d_splitters uint64 [n_parts - 1] on the device; copies the accumulated, unthresholded
 *                              table (ascending codes) to d_codes_out / d_counts_out uint64 (device, or both NULL for
 *                              the offsets only) and writes the host offsets part_off_out int64 [n_parts + 1]: part p =
 *                              codes in [splitters[p - 1], splitters[p]) at part_off_out[p] .. part_off_out[p + 1].
 *                              The table stays as it is.
 *   fdr_kmer_count_merge_dev:  n_runs (1 .. 256) runs at run_off[r] .. run_off[r + 1] (host int64 [n_runs + 1],
 *                              run_off[0] = 0) of d_codes / d_counts uint64 (device), each strictly ascending in code;
 *                              sums the counts of equal codes, keeps totals >= min_count and leaves them in the
 *                              context: *n_out = their number, then fdr_kmer_count_fetch (ascending code order).  One
 *                              pass (tile boundaries from samples of every run, every element placed by its bounds in
 *                              the other runs), not a chain of pairwise merges.  Fewer than 2^31 entries in all.
 *   fdr_kmer_count_merge:      the same from host arrays (replaces the context's accumulated table).
 * stream: a hipStream_t (NULL = the context's). */
int fdr_kmer_count_export_dev(fdr_ctx *ctx, const uint64_t *d_splitters, int32_t n_parts, uint64_t *d_codes_out,
                              uint64_t *d_counts_out, int64_t *part_off_out, void *stream);
int fdr_kmer_count_merge_dev(fdr_ctx *ctx, int32_t n_runs, const int64_t *run_off, const uint64_t *d_codes,
                             const uint64_t *d_counts, int64_t min_count, int64_t *n_out, void *stream);
int fdr_kmer_count_merge(fdr_ctx *ctx, int32_t n_runs, const int64_t *run_off, const uint64_t *codes,
                         const uint64_t *counts, int64_t min_count, int64_t *n_out);

/* ---- FASTA / FASTQ reader of the k-mer stage (host only: no context, no GPU) -------------------------
 * Replaces read_sequences of kmer_searcher/kmer_searcher.cpp:153-200 (FASTQ iff the first line starts with '@';
 * FASTA id = header up to the first space or tab, sequence = the following non-empty lines with only the '\n'
 * removed, records with an empty id and anything before the first header dropped; FASTQ id = the header line
 * after '@', sequence = the next line, two lines skipped) for a PIECE of the file: raw[0, n) = the unconsumed
 * tail of the previous piece followed by new bytes, eof = nothing follows.  fastq_ids_as_fasta: the pipeline's
 * `seqkit fq2fa` step (fedrann/count_kmers.py:76-79) -- FASTQ names cut like FASTA ids, empty names dropped.
 *   fdr_reads_scan:  consumed = bytes holding whole records only (the rest waits for the next piece), their
 *                    record count and total sequence length;
 *   fdr_reads_parse: seqs [n_bases], seq_off int64 [n_records + 1], id_span int64 [2 n_records] = (begin, end)
 *                    of each id inside raw; FDR_E_STATE if raw[0, consumed) no longer matches the scan. */
int fdr_reads_scan(const uint8_t *raw, int64_t n, int32_t is_fastq, int32_t fastq_ids_as_fasta, int32_t eof,
                   int64_t *consumed, int64_t *n_records, int64_t *n_bases);
int fdr_reads_parse(const uint8_t *raw, int64_t consumed, int32_t is_fastq, int32_t fastq_ids_as_fasta,
                    int64_t n_records, int64_t n_bases, uint8_t *seqs, int64_t *seq_off, int64_t *id_span);

/* ---- kmer_searcher output.bin -> doubled binary CSR (host only: no context, no GPU) ---------------
 * Replaces fedrann/feature_extraction.py:108-140 (parse_kmer_searcher_output: header '<4sB3sQ' =
 * "KMER", version 1, record count; per record '<H' id length, id bytes, '<I' index count, that many
 * '<Q' feature indices; a record yields its index set and the strand mirror i + L if i < L else i - L,
 * L = n_features / 2) together with the COO -> CSR conversion of :191-204 (ascending columns per row).
 * Row 2r = record r, row 2r + 1 = its mirror.  Two calls, caller-allocated outputs:
 *   fdr_kmer_output_scan: record count R, sum of index counts nnz, sum of id lengths;
 *   fdr_kmer_output_load: indptr int64 [2R + 1], indices int32 [2 nnz], name_off int64 [R + 1],
 *                         names [name_bytes] (raw id bytes, record r at name_off[r] .. name_off[r+1]);
 *                         n_records / nnz / name_bytes = the scan's results the arrays were sized from
 *                         (FDR_E_STATE if the file no longer matches them: nothing is written then).
 * n_threads <= 0: all hardware threads.  Errors as in the reference (bad magic / version, short
 * header -> FDR_E_ARG), plus truncated records, indices outside [0, n_features) and repeated indices
 * inside a record (the reference would sum them; kmer_searcher emits sets). */
int fdr_kmer_output_scan(const char *path, int64_t *n_records, int64_t *nnz, int64_t *name_bytes);
int fdr_kmer_output_load(const char *path, int64_t n_features, int32_t n_threads, int64_t n_records, int64_t nnz,
                         int64_t name_bytes, int64_t *indptr, int32_t *indices, int64_t *name_off, char *names);
/* The same for the records [rec_lo, rec_hi) only -- one rank's row block of a row-sharded run (rows 2 rec_lo ..
 * 2 rec_hi of the matrix), so that G ranks hold 1/G of the CSR each instead of G copies of it:
 *   fdr_kmer_output_scan_range: record count of the FILE, sum of index counts of the RANGE, id bytes of the file;
 *   fdr_kmer_output_load_range: indptr int64 [2 (rec_hi - rec_lo) + 1] (rebased to 0), indices int32 [2 nnz_range];
 *                               name_off int64 [R + 1] + names of ALL records (the writer names any target row),
 *                               or name_off = NULL for no names. */
int fdr_kmer_output_scan_range(const char *path, int64_t rec_lo, int64_t rec_hi, int64_t *n_records,
                               int64_t *nnz_range, int64_t *name_bytes);
int fdr_kmer_output_load_range(const char *path, int64_t n_features, int32_t n_threads, int64_t n_records,
                               int64_t rec_lo, int64_t rec_hi, int64_t nnz_range, int64_t name_bytes, int64_t *indptr,
                               int32_t *indices, int64_t *name_off, char *names);

/* The writer of the same file, a group of records at a time (kmer_searcher/kmer_searcher.cpp:106-128: '<H' id
 * length, id, '<I' count, the indices as '<Q'): appends n_records records to `path`, record r with the id
 * names[name_off[r] .. name_off[r+1]) and the indices indices[indptr[r] .. indptr[r+1]).  Ids must be printable
 * ASCII as there (:113-117) and at most 65535 bytes (FDR_E_ARG before anything is written).  The caller writes
 * the 16-byte header and patches its record count. */
int fdr_kmer_output_append(const char *path, int64_t n_records, const int64_t *name_off, const char *names,
                           const int64_t *indptr, const int32_t *indices);

/* ---- overlaps.tsv writer (host only: no context, no GPU) ---------------------------------------------
 * Replaces get_output_dataframe + DataFrame.to_csv(sep="\t", index=False) (fedrann/__main__.py:261-300,
 * :385): for every row q = row0 + r (r < n_rows) and column c with target t = idx[r][c], in that order,
 * unless t == q:   name[q] \t "+-"[strand[q]] \t name[t] \t "+-"[strand[t]] \t c \t dist[r][c] \n
 * byte for byte what pandas writes for the reference's DataFrame (float32 distances in their shortest
 * round-trip form, numpy layout; a negative t aliases from the end like Python indexing).  idx / dist
 * [n_rows, k] are the rows row0 .. row0 + n_rows of the neighbour graph (a rank's block of a row-sharded
 * run); names / name_off / strands describe all n_total rows -- or, with strands == NULL, names / name_off describe
 * the n_total / 2 RECORDS of a fwd / rev doubled matrix (feature_extraction.py:136-140): row t carries record t >> 1's
 * id and strand t & 1, and no id is held twice.  append: open the file for appending;
 * write_header: the column-name line first.  n_threads <= 0: all hardware threads.  *lines_out (may be
 * NULL) = data lines written. */
int fdr_overlaps_write(const char *path, int32_t append, int32_t write_header, int64_t n_total, int64_t row0,
                       int64_t n_rows, int32_t k, const int32_t *idx, const float *dist, const int64_t *name_off,
                       const char *names, const uint8_t *strands, int32_t n_threads, int64_t *lines_out);

/* The same writer for ragged rows (the result of a radius search): row r's entries are idx / dist [indptr[r],
 * indptr[r + 1]) instead of [r k, (r + 1) k); indptr int64 [n_rows + 1], monotone, indptr[0] >= 0.  Everything else
 * is fdr_overlaps_write, through the same line formatter: the entry at position c of its row (a skipped self entry
 * counts) is written with neighbor_rank c.  A CSR whose rows all have k entries gives fdr_overlaps_write's bytes.
 * Host only. */
int fdr_overlaps_write_csr(const char *path, int32_t append, int32_t write_header, int64_t n_total, int64_t row0,
                           int64_t n_rows, const int64_t *indptr, const int32_t *idx, const float *dist,
                           const int64_t *name_off, const char *names, const uint8_t *strands, int32_t n_threads,
                           int64_t *lines_out);

#ifdef __cplusplus
}
#endif
#endif /* FEDRANN_HIP_H */
