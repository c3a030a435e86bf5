// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit) behind knn_sparse.inc, ahead of the two
// radius searches.
// ------------------------------------------------------------------------------------------
// The protocol of a radius call, once, for knn_sparse_radius.inc (R1 .. R3) and knn_dense_radius.inc (D-R1 .. D-R3):
// count, scan, indptr_out, the cap, emit into the counted segments, sort, split, cross-check, hold (DESIGN.md section
// 5 lists the steps).  A search supplies its passes and its sort; the frame is the functions below, in call order, all
// on a RadiusResult (fedrann_hip.hip) with the owner's rocprim storage.
// ------------------------------------------------------------------------------------------
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

// ---- device side ----------------------------------------------------------------------------------------------------
// The segment [seg0, seg0 + seg) of a zero query: the list of the index's nzero zero rows, each at distance bits 0,
// as far as the segment reaches; a segment of another length is a mismatch.  One wave, `lane` of it.  The sparse
// search's emit pass calls it; dr_exact_kernel spells the same branch out (its register count moved with the call).
__device__ __forceinline__ void radius_emit_zero(int lane, long long seg0, long long seg, long long nzero,
                                                 const int *__restrict__ zlist, u64 *__restrict__ keys,
                                                 u64 *__restrict__ flags) {
    for (long long i = lane; i < min(nzero, seg); i += 64) keys[seg0 + i] = (u64)(unsigned)zlist[i];
    if (lane == 0 && seg != nzero) atomicAdd(&flags[RR_FLAG_MISMATCH], 1ull);
}

// the nonzero bytes of flag[0, n), added to *counter: one atomic per wave that found any
__global__ __launch_bounds__(256) void radius_count_flags_kernel(long long n, const unsigned char *__restrict__ flag,
                                                                 u64 *__restrict__ counter) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const u64 m = __ballot(i < n && flag[i] != 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (u64)__popcll(m));
}

// The split.  COMPACT (the dense search's D-R3; dst_off / src_off [nseg + 1] each) compacts as it splits: output entry
// i belongs to the segment s with dst_off[s] <= i < dst_off[s + 1] and is the key at src_off[s] + (i - dst_off[s]),
// the first dst_off[s + 1] - dst_off[s] keys of each source segment.  The sparse search's instantiation, COMPACT =
// false, reads key i and none of the three.
template <bool COMPACT>
__global__ __launch_bounds__(256) void radius_split_kernel(long long total, const u64 *__restrict__ keys,
                                                           int *__restrict__ idx, float *__restrict__ dist,
                                                           long long nseg, const long long *__restrict__ dst_off,
                                                           const long long *__restrict__ src_off) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    long long src = i;
    if constexpr (COMPACT) {
        long long lo = 0, hi = nseg;  // the last s in [0, nseg) with dst_off[s] <= i (dst_off[0] = 0 <= i < dst_off[nseg])
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (dst_off[mid] <= i) lo = mid;
            else hi = mid;
        }
        src = src_off[lo] + (i - dst_off[lo]);
    }
    const u64 key = keys[src];
    idx[i] = (int)(unsigned)key;
    dist[i] = __uint_as_float((unsigned)(key >> 32));
}

// ---- host side ----------------------------------------------------------------------------------------------------
// what the steps of one call share: the stream, the entry point's name in messages, the queries, the cap, the indptr
struct RadiusCall {
    hipStream_t st;
    const char *who;
    int64_t nq, max_hits;
    int64_t *indptr_out;
};

// What every radius entry checks alike, before anything else: the index (`kind`: "sparse" / "dense"), the radius, the
// cap.  `ranks` names the function that ranks all rows, which a bound of 1 would ask for.
static int radius_args(bool have_index, const char *who, const char *kind, const char *ranks, float radius,
                       int64_t max_hits) {
    if (!have_index) return fail(FDR_E_STATE, "%s: the context holds no %s index", who, kind);
    const bool all = radius >= 1.0f;  // (a NaN is neither in range nor `all`)
    if (all || !(radius >= 0.0f))
        return fail(FDR_E_ARG, "%s: the radius must be in [0, 1), got %g%s%s%s", who, (double)radius,
                    all ? ": every row is within 1 of every query, and " : "", all ? ranks : "", all ? " ranks them" : "");
    if (max_hits < 1 || max_hits > INT32_MAX)
        return fail(FDR_E_ARG, "%s: max_hits (%lld) must be in [1, 2^31)", who, (long long)max_hits);
    return FDR_OK;
}

// a call without queries: an empty result, held
static int radius_none(RadiusResult &rr, int64_t *indptr_out) {
    indptr_out[0] = 0;
    rr.held = 0;
    return FDR_OK;
}

// count / off / flags for the call's queries, count (a 0 behind the last query's) and flags cleared
static int radius_reserve(RadiusResult &rr, const RadiusCall &c) {
    int rc;
    rr.counted = 0;
    if ((rc = rr.count.reserve((size_t)c.nq + 1))) return rc;
    if ((rc = rr.off.reserve((size_t)c.nq + 1))) return rc;
    if ((rc = rr.flags.reserve(RR_FLAGS))) return rc;
    HIP_TRY(hipMemsetAsync(rr.count.ptr(), 0, ((size_t)c.nq + 1) * 8, c.st));
    HIP_TRY(hipMemsetAsync(rr.flags.ptr(), 0, RR_FLAGS * 8, c.st));
    return FDR_OK;
}

// count -> to: the exclusive scan over the nq + 1 entries, to[nq] the total
static int radius_scan(RadiusResult &rr, DevArray<char> &tmp, const RadiusCall &c, long long *to) {
    auto scan = [&](void *t, size_t &bytes) {
        return rocprim::exclusive_scan(t, bytes, rr.count.ptr(), to, 0ll, (size_t)c.nq + 1, rocprim::plus<long long>(),
                                       c.st);
    };
    return rocprim_run(tmp, "rocprim::exclusive_scan", scan);
}

// The counts' scan in `off` and in indptr_out, on the host when this returns; flags_out (or null): the RR_FLAGS flag
// words with it, in the same synchronisation.  rr.counted (0 until then) is the total, `what` its word in the refusal
// ("hits" / "candidates") and `holds` what that says indptr_out holds.  FDR_OK with rr.counted > 0: keys and sorted
// hold that many entries; with rr.counted == 0 the call is over, its empty result held.
static int radius_offsets(RadiusResult &rr, DevArray<char> &tmp, const RadiusCall &c, const char *what,
                          const char *holds, u64 *flags_out) {
    int rc;
    if ((rc = radius_scan(rr, tmp, c, rr.off.ptr()))) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "the scan is the result's indptr");
    HIP_TRY(hipMemcpyAsync(c.indptr_out, rr.off.ptr(), ((size_t)c.nq + 1) * 8, hipMemcpyDeviceToHost, c.st));
    if (flags_out) HIP_TRY(hipMemcpyAsync(flags_out, rr.flags.ptr(), RR_FLAGS * 8, hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    const long long total = rr.counted = c.indptr_out[c.nq];
    if (total > c.max_hits)  // (the one refusal that has written its output: the caller cuts the block by the counts)
        return fail(FDR_E_ARG, "%s: %lld %s exceed max_hits = %lld (indptr_out holds the %s: search fewer rows per call)",
                    c.who, total, what, (long long)c.max_hits, holds);
    if (total == 0) {
        rr.held = 0;
        return FDR_OK;
    }
    if ((rc = rr.keys.reserve((size_t)total))) return rc;
    return rr.sorted.reserve((size_t)total);
}

// zlist = the rows with zero[row] != 0 among the index's n, in index order; RR_FLAG_ZLIST = their number (radius_check)
static int radius_zero_list(RadiusResult &rr, DevArray<char> &tmp, const RadiusCall &c, const unsigned char *zero,
                            int64_t n, long long nzero) {
    if (int rc = rr.zlist.reserve((size_t)nzero)) return rc;
    auto select = [&](void *t, size_t &bytes) {
        return rocprim::select(t, bytes, rocprim::counting_iterator<int>(0), zero, rr.zlist.ptr(),
                               rr.flags.ptr() + RR_FLAG_ZLIST, (size_t)n, c.st);
    };
    return rocprim_run(tmp, "rocprim::select", select);
}

// the flags behind the last pass, with a synchronisation: no mismatch and, where the call `listed` the zero rows, all nzero
static int radius_check(RadiusResult &rr, const RadiusCall &c, bool listed, long long nzero) {
    u64 f[RR_FLAGS] = {};
    HIP_TRY(hipMemcpyAsync(f, rr.flags.ptr(), RR_FLAGS * 8, hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    if (f[RR_FLAG_MISMATCH] != 0 || (listed && f[RR_FLAG_ZLIST] != (u64)nzero))
        return fail(FDR_E_HIP, "internal: %s: the emit pass disagrees with the count pass on %llu queries (zero rows "
                    "listed: %llu of %lld)", c.who, (unsigned long long)f[RR_FLAG_MISMATCH],
                    (unsigned long long)f[RR_FLAG_ZLIST], nzero);
    return FDR_OK;
}

// the body of both fetches, behind use_device; `next` names the call that drops a held result
static int radius_fetch(hipStream_t st, RadiusResult &rr, const char *who, const char *next, int64_t hits,
                        int32_t *idx_out, float *dist_out) {
    if (rr.held < 0)
        return fail(FDR_E_STATE, "%s: the context holds no radius result (the %s after a radius search drops it)", who,
                    next);
    if (hits != rr.held)
        return fail(FDR_E_ARG, "%s: hits = %lld, the held result has %lld", who, (long long)hits, rr.held);
    if (hits == 0) return FDR_OK;
    if (!idx_out || !dist_out) return fail(FDR_E_ARG, "%s: null pointer", who);
    HIP_TRY(hipMemcpyAsync(idx_out, rr.idx(), (size_t)hits * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dist_out, rr.dist(), (size_t)hits * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return FDR_OK;
}
