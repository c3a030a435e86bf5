// Part of libfedrann_hip.so (included by fedrann_hip.hip).
//
// fdr_radius_merge: the exact merge of the per-rank ragged rows of a target-sharded sparse radius search
// (fedrann_amd.distributed.sparse_radius_sharded).  Each of n_parts ranks has searched its own targets for the same nq
// queries and holds, per query, every one of ITS targets within the radius, ascending by key = distance bits << 32 |
// global index; a query's answer is the union of its n_parts rows in key order.  Why that is the one-GPU search's answer
// under every sparse rule is argued in the docstring of distributed.merge_sparse_radius, which stays the model of this
// file and the route without a GPU.  fdr_topk_merge's contract (topk_merge.inc) carried to rows of any length: the keys,
// the three rules of the check and the refusal record are its own.
//
// M1  radius_merge_kernel: one wave per 64 entries of a query.  A query's entries are counted part after part (part
//     0's row, then part 1's, ...); the host, which walks the indptrs anyway, lists the work items (query, chunk of 64)
//     of every query that has entries, so a row of 160 000 entries is 2 500 waves and not one wave's 2 500 strides, and
//     a row of 20 entries per part fills its lanes across the parts.  Lane p < n_parts holds the start and the length
//     of row (p, q); the wave reads them by lane, first to find each lane's own (part, position), then to place.
//   check  index >= 0, distance bits <= 0x7f800000, the entry's key above its predecessor's in the row.  A wave that
//          finds a violation records the smallest (query, part, rule) it saw with one atomicMin and places nothing;
//          the host reads the record back before it copies any result out (what other waves have placed by then is in
//          the context's buffers only).
//   place  no sort and no heads to advance: the entry at position j of row (p, q) goes to
//              indptr_out[q] + j + sum over p' < p of #{keys of row (p', q) <= key} + sum over p' > p of #{... < key},
//          each count a binary search in the other part's row (an empty row costs nothing).  Inside a strictly
//          ascending row the positions are distinct, and "<=" towards the lower parts, "<" towards the higher ones
//          orders equal keys of two parts by part: a bijection onto the output row, the lower part's entry first.
// No LDS; the only atomic is the refusal record's.  The work is flat over the entries: each costs (n_parts - 1) searches
// of log2(row length) steps, two 4-byte loads a step.  Every load is inside [0, total) and every store inside the
// query's output row, whatever the entries hold: the host has checked the indptrs before the upload, and a count is
// at most its row's length.

constexpr int RM_WAVES = 4;  // waves (work items) per workgroup

// #{keys of the ascending row [at, at + len) that are < bound}
__device__ __forceinline__ int rm_count(const int *__restrict__ idx, const float *__restrict__ dist, int at, int len,
                                        u64 bound) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tm_key(idx[at + mid], dist[at + mid]) < bound) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// items int2 [n_items]: (query, chunk) -- the entries [64 * chunk, 64 * chunk + 64) of the query, counted part after
// part.  starts int32 [n_parts, nq + 1]: row (p, q) is the entries [starts[p][q], starts[p][q + 1]) of idx_parts /
// dist_parts (the part's indptr plus the entries of the parts before it); indptr_out int32 [nq + 1].
__global__ __launch_bounds__(64 * RM_WAVES) void radius_merge_kernel(
    int n_items, int nq, int n_parts, const int2 *__restrict__ items, const int *__restrict__ starts,
    const int *__restrict__ indptr_out, const int *__restrict__ idx_parts, const float *__restrict__ dist_parts,
    int *__restrict__ idx_out, float *__restrict__ dist_out, u64 *__restrict__ refusal) {
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * RM_WAVES + (threadIdx.x >> 6);
    if (item >= n_items) return;  // (wave-uniform)
    const int2 it = items[item];
    const int q = it.x, e = it.y * 64 + lane;
    int row_at = 0, row_len = 0;
    if (lane < n_parts) {
        const int *s = starts + (size_t)lane * ((size_t)nq + 1) + (size_t)q;
        row_at = s[0];
        row_len = s[1] - row_at;
    }
    // ---- this lane's entry: position j of row (p, q), at `at + j` ----
    int p = -1, j = 0, at = 0, before = 0;
    for (int o = 0; o < n_parts; ++o) {
        const int o_at = __shfl(row_at, o, 64), o_len = __shfl(row_len, o, 64);
        if (p < 0 && e < before + o_len) {
            p = o;
            j = e - before;
            at = o_at;
        }
        before += o_len;
    }
    const bool live = p >= 0;  // (the query's last chunk may be short)
    const int index = live ? idx_parts[at + j] : 0;
    const float dist = live ? dist_parts[at + j] : 0.0f;
    const u64 key = tm_key(index, dist);
    // ---- check ----
    u64 bad = TM_NONE;
    if (live) {
        int rule = 0;
        if (index < 0) rule = TM_RULE_INDEX;
        else if (__float_as_uint(dist) > 0x7f800000u) rule = TM_RULE_DISTANCE;
        else if (j > 0 && tm_key(idx_parts[at + j - 1], dist_parts[at + j - 1]) >= key) rule = TM_RULE_ORDER;
        if (rule) bad = ((u64)q << 16) | ((u64)p << 8) | (u64)rule;
    }
    if (__ballot(bad != TM_NONE)) {
        bad = tm_wave_min(bad, 64);
        if (lane == 0) atomicMin(refusal, bad);
        return;
    }
    // ---- place ----
    int pos = indptr_out[q] + j;
    for (int o = 0; o < n_parts; ++o) {
        const int o_at = __shfl(row_at, o, 64), o_len = __shfl(row_len, o, 64);
        if (!live || o == p || o_len == 0) continue;
        pos += rm_count(idx_parts, dist_parts, o_at, o_len, key + (u64)(o < p));  // (o < p: the keys <= key)
    }
    if (live) {
        idx_out[pos] = index;
        dist_out[pos] = dist;
    }
}

FDR_EXPORT int fdr_radius_merge(fdr_ctx *ctx, int64_t nq, int32_t n_parts, const int64_t *indptr_parts,
                                const int32_t *idx_parts, const float *dist_parts, int64_t *indptr_out, int32_t *idx_out,
                                float *dist_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (n_parts < 1 || n_parts > TM_MAX_PARTS)
        return fail(FDR_E_ARG, "radius_merge: n_parts=%d unsupported (1..%d)", n_parts, TM_MAX_PARTS);
    if (nq < 0 || nq > INT32_MAX) return fail(FDR_E_ARG, "radius_merge: nq (%lld) must be in [0, 2^31)", (long long)nq);
    if (!indptr_parts || !indptr_out) return fail(FDR_E_ARG, "radius_merge: null indptr pointer");
    // ---- the indptrs, on the host: what keeps the kernel's loads in bounds ----
    const size_t rows = (size_t)nq + 1;
    int64_t total = 0;
    for (int p = 0; p < n_parts; ++p) {
        const int64_t *ip = indptr_parts + (size_t)p * rows;
        if (ip[0] != 0) return fail(FDR_E_ARG, "radius_merge: part %d: its indptr starts at %lld, not 0", p, (long long)ip[0]);
        for (size_t q = 0; q < (size_t)nq; ++q)
            if (ip[q + 1] < ip[q])
                return fail(FDR_E_ARG, "radius_merge: part %d, query %zu: the indptr decreases", p, q);
        if (ip[nq] > INT32_MAX - total)
            return fail(FDR_E_ARG, "radius_merge: the parts hold 2^31 entries or more in all");
        total += ip[nq];
    }
    if (total == 0 || nq == 0) {  // (nothing to merge: the indptr alone)
        for (size_t q = 0; q < rows; ++q) indptr_out[q] = 0;
        return FDR_OK;
    }
    if (!idx_parts || !dist_parts || !idx_out || !dist_out) return fail(FDR_E_ARG, "radius_merge: null pointer");
    RadiusMergeScratch &rm = ctx->rm;
    rm.h_starts.resize((size_t)n_parts * rows);
    rm.h_indptr_out.assign(rows, 0);
    rm.h_items.clear();
    int64_t base = 0;
    for (int p = 0; p < n_parts; ++p) {
        const int64_t *ip = indptr_parts + (size_t)p * rows;
        int *s = rm.h_starts.data() + (size_t)p * rows;
        for (size_t q = 0; q < rows; ++q) {
            s[q] = (int)(base + ip[q]);
            rm.h_indptr_out[q] += (int)ip[q];
        }
        base += ip[nq];
    }
    for (size_t q = 0; q < (size_t)nq; ++q)  // the work items: 64 entries of a query each
        for (int c = 0, left = rm.h_indptr_out[q + 1] - rm.h_indptr_out[q]; left > 0; ++c, left -= 64)
            rm.h_items.push_back(make_int2((int)q, c));
    const size_t n_items = rm.h_items.size();  // (at most total / 64 + nq: below 2^31 + 2^25)
    if (n_items > (size_t)INT32_MAX) return fail(FDR_E_ARG, "radius_merge: 2^31 work items or more (%zu)", n_items);
    const hipStream_t st = ctx->stream;
    const size_t n = (size_t)total;
    if ((rc = rm.starts.reserve((size_t)n_parts * rows))) return rc;
    if ((rc = rm.indptr_out.reserve(rows))) return rc;
    if ((rc = rm.items.reserve(n_items))) return rc;
    if ((rc = rm.idx_parts.reserve(n))) return rc;
    if ((rc = rm.dist_parts.reserve(n))) return rc;
    if ((rc = rm.idx_out.reserve(n))) return rc;
    if ((rc = rm.dist_out.reserve(n))) return rc;
    if ((rc = rm.refusal.reserve(1))) return rc;
    HIP_TRY(upload(rm.starts, rm.h_starts.data(), (size_t)n_parts * rows, st));
    HIP_TRY(upload(rm.indptr_out, rm.h_indptr_out.data(), rows, st));
    HIP_TRY(upload(rm.items, rm.h_items.data(), n_items, st));
    HIP_TRY(upload(rm.idx_parts, idx_parts, n, st));
    HIP_TRY(upload(rm.dist_parts, dist_parts, n, st));
    HIP_TRY(hipMemsetAsync(rm.refusal.ptr(), 0xff, 8, st));
    hipLaunchKernelGGL(radius_merge_kernel, dim3((unsigned)((n_items + RM_WAVES - 1) / RM_WAVES)), dim3(64 * RM_WAVES), 0,
                       st, (int)n_items, (int)nq, n_parts, rm.items.ptr(), rm.starts.ptr(), rm.indptr_out.ptr(), rm.idx_parts.ptr(), rm.dist_parts.ptr(),
                       rm.idx_out.ptr(), rm.dist_out.ptr(), rm.refusal.ptr());
    HIP_TRY(hipGetLastError());
    u64 refused = TM_NONE;
    HIP_TRY(download(&refused, rm.refusal, 1, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (refused != TM_NONE) {  // (nothing has been written to indptr_out / idx_out / dist_out)
        const int rule = (int)(refused & 0xff), part = (int)((refused >> 8) & 0xff);
        const long long query = (long long)(refused >> 16);
        const char *what = rule == TM_RULE_INDEX      ? "a negative index"
                           : rule == TM_RULE_DISTANCE ? "a distance that is negative or NaN (its bits must be at most 0x7f800000)"
                                                      : "the row is not strictly ascending by (distance bits, index)";
        return fail(FDR_E_ARG, "radius_merge: part %d, query %lld: %s", part, query, what);
    }
    HIP_TRY(download(idx_out, rm.idx_out, n, st));
    HIP_TRY(download(dist_out, rm.dist_out, n, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t q = 0; q < rows; ++q) indptr_out[q] = rm.h_indptr_out[q];
    return FDR_OK;
}
