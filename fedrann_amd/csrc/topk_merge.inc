// Part of libfedrann_hip.so (included by fedrann_hip.hip).
//
// fdr_topk_merge: the exact merge of the per-rank candidate lists of a target-sharded sparse search
// (fedrann_amd.distributed.sparse_knn_sharded).  Each of n_parts ranks has searched its own targets for the same nq
// queries and holds kp candidates per query, ascending by key = distance bits << 32 | global index; a query's answer is
// the first k keys of the union of its n_parts rows.  Why that is the one-GPU search's answer under every sparse rule is
// proven in the docstring of distributed.merge_sparse_topk, which stays the model of this file and the route without a
// GPU.
//
// T1  topk_merge_kernel: one wave per query, in two steps.
//   check  the wave walks the query's n_parts x kp entries once, consecutive lanes on consecutive entries of a part's
//          row: index >= 0, distance bits <= 0x7f800000 (sign clear, no NaN: bit order is then value order), each entry's
//          key above its predecessor's in the row.  A wave that finds a violation records the smallest (query, part, rule)
//          it saw with one atomicMin and merges nothing; the host reads the record back before it copies any result out.
//   merge  lane p < n_parts owns part p: it holds the key at the head of its row and the one behind it (loaded a round
//          early), an exhausted part the all-ones key, which no valid entry equals.  k rounds: the minimum over the lanes
//          by a butterfly over the next power of two of n_parts lanes, the lowest lane among equals advances (equal keys
//          in two parts are a duplicate index, the caller's broken promise: both come out, the lower part first), lane
//          r & 63 keeps round r's key.  The results leave the registers at the end, consecutive lanes on consecutive slots.
// No LDS; the only atomic is the refusal record's.  The kernel reads 8 bytes per entry once (the merge's loads hit the
// lines the check brought in): its cost is the upload of the parts, which is why they are taken part-major, as a
// gather by source rank leaves them.

enum { TM_RULE_INDEX = 1, TM_RULE_DISTANCE = 2, TM_RULE_ORDER = 3 };
constexpr int TM_WAVES = 4;        // waves (queries) per workgroup
constexpr int TM_MAX_PARTS = 64;   // one lane per part
constexpr u64 TM_NONE = ~0ull;     // the exhausted part's key; the refusal record of a call that refuses nothing

__device__ __forceinline__ u64 tm_key(int index, float dist) {
    return ((u64)__float_as_uint(dist) << 32) | (unsigned)index;
}

// the minimum of v over the lanes [0, span), span a power of two <= 64, in every lane of the wave
__device__ __forceinline__ u64 tm_wave_min(u64 v, int span) {
    for (int off = 1; off < span; off <<= 1) {
        const u64 o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(64 * TM_WAVES) void topk_merge_kernel(
    long long nq, int n_parts, int kp, int k, const int *__restrict__ idx_parts, const float *__restrict__ dist_parts,
    int *__restrict__ idx_out, float *__restrict__ dist_out, u64 *__restrict__ refusal) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * TM_WAVES + (threadIdx.x >> 6);
    if (q >= nq) return;  // (wave-uniform)
    // ---- check ----
    u64 bad = TM_NONE;
    const int entries = n_parts * kp;  // (at most 64 * FDR_MAX_K)
    for (int e = lane; e < entries; e += 64) {
        const int p = e / kp, j = e - p * kp;
        const size_t at = ((size_t)p * (size_t)nq + (size_t)q) * (size_t)kp + (size_t)j;
        const int index = idx_parts[at];
        const float dist = dist_parts[at];
        int rule = 0;
        if (index < 0) rule = TM_RULE_INDEX;
        else if (__float_as_uint(dist) > 0x7f800000u) rule = TM_RULE_DISTANCE;
        else if (j > 0 && tm_key(idx_parts[at - 1], dist_parts[at - 1]) >= tm_key(index, dist)) rule = TM_RULE_ORDER;
        if (rule) {
            const u64 code = ((u64)q << 16) | ((u64)p << 8) | (u64)rule;
            bad = code < bad ? code : bad;
        }
    }
    if (__ballot(bad != TM_NONE)) {
        bad = tm_wave_min(bad, 64);
        if (lane == 0) atomicMin(refusal, bad);
        return;
    }
    // ---- merge ----
    int span = 1;
    while (span < n_parts) span <<= 1;
    const bool own = lane < n_parts;
    const size_t row = own ? ((size_t)lane * (size_t)nq + (size_t)q) * (size_t)kp : 0;
    const int *ip = idx_parts + row;
    const float *dp = dist_parts + row;
    u64 head = own ? tm_key(ip[0], dp[0]) : TM_NONE;
    u64 next = own && kp > 1 ? tm_key(ip[1], dp[1]) : TM_NONE;
    int pos = 0;
    u64 out0 = 0, out1 = 0;
    for (int r = 0; r < k; ++r) {
        const u64 m = tm_wave_min(head, span);
        const int winner = __ffsll((long long)__ballot(head == m)) - 1;
        if (lane == (r & 63)) {
            if (r < 64) out0 = m;
            else out1 = m;
        }
        if (lane == winner) {
            head = next;
            ++pos;
            next = pos + 1 < kp ? tm_key(ip[pos + 1], dp[pos + 1]) : TM_NONE;
        }
    }
    const size_t o = (size_t)q * (size_t)k;
    if (lane < k) {
        idx_out[o + lane] = (int)(unsigned)out0;
        dist_out[o + lane] = __uint_as_float((unsigned)(out0 >> 32));
    }
    if (lane + 64 < k) {
        idx_out[o + lane + 64] = (int)(unsigned)out1;
        dist_out[o + lane + 64] = __uint_as_float((unsigned)(out1 >> 32));
    }
}

FDR_EXPORT int fdr_topk_merge(fdr_ctx *ctx, int64_t nq, int32_t n_parts, int32_t kp, int32_t k, const int32_t *idx_parts,
                              const float *dist_parts, int32_t *idx_out, float *dist_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (k < 1 || k > FDR_MAX_K) return fail(FDR_E_ARG, "topk_merge: k=%d unsupported (1..%d)", k, FDR_MAX_K);
    if (kp < 1 || kp > FDR_MAX_K) return fail(FDR_E_ARG, "topk_merge: kp=%d unsupported (1..%d)", kp, FDR_MAX_K);
    if (n_parts < 1 || n_parts > TM_MAX_PARTS)
        return fail(FDR_E_ARG, "topk_merge: n_parts=%d unsupported (1..%d)", n_parts, TM_MAX_PARTS);
    if ((int64_t)n_parts * kp < k)
        return fail(FDR_E_ARG, "topk_merge: %d parts of %d candidates hold fewer than k = %d", n_parts, kp, k);
    if (nq < 0 || nq > INT32_MAX) return fail(FDR_E_ARG, "topk_merge: nq (%lld) must be in [0, 2^31)", (long long)nq);
    if (nq * kp > INT32_MAX || nq * k > INT32_MAX)
        return fail(FDR_E_ARG, "topk_merge: %lld queries of %d candidates per part, %d results: an array of 2^31 "
                    "elements or more", (long long)nq, kp, k);
    if (nq == 0) return FDR_OK;
    if (!idx_parts || !dist_parts || !idx_out || !dist_out) return fail(FDR_E_ARG, "topk_merge: null pointer");
    TopkMergeScratch &tm = ctx->tm;
    const hipStream_t st = ctx->stream;
    const size_t n_in = (size_t)n_parts * (size_t)nq * (size_t)kp, n_out = (size_t)nq * (size_t)k;
    if ((rc = tm.idx_parts.reserve(n_in))) return rc;
    if ((rc = tm.dist_parts.reserve(n_in))) return rc;
    if ((rc = tm.idx_out.reserve(n_out))) return rc;
    if ((rc = tm.dist_out.reserve(n_out))) return rc;
    if ((rc = tm.refusal.reserve(1))) return rc;
    HIP_TRY(hipMemcpyAsync(tm.idx_parts.ptr(), idx_parts, n_in * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(tm.dist_parts.ptr(), dist_parts, n_in * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(tm.refusal.ptr(), 0xff, 8, st));
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((nq + TM_WAVES - 1) / TM_WAVES)), dim3(64 * TM_WAVES), 0, st,
                       (long long)nq, n_parts, kp, k, tm.idx_parts.ptr(), tm.dist_parts.ptr(), tm.idx_out.ptr(),
                       tm.dist_out.ptr(), tm.refusal.ptr());
    HIP_TRY(hipGetLastError());
    u64 refused = TM_NONE;
    HIP_TRY(hipMemcpyAsync(&refused, tm.refusal.ptr(), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (refused != TM_NONE) {  // (nothing has been written to idx_out / dist_out)
        const int rule = (int)(refused & 0xff), part = (int)((refused >> 8) & 0xff);
        const long long query = (long long)(refused >> 16);
        const char *what = rule == TM_RULE_INDEX      ? "a negative index"
                           : rule == TM_RULE_DISTANCE ? "a distance that is negative or NaN (its bits must be at most 0x7f800000)"
                                                      : "the row is not strictly ascending by (distance bits, index)";
        return fail(FDR_E_ARG, "topk_merge: part %d, query %lld: %s", part, query, what);
    }
    HIP_TRY(hipMemcpyAsync(idx_out, tm.idx_out.ptr(), n_out * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dist_out, tm.dist_out.ptr(), n_out * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return FDR_OK;
}
