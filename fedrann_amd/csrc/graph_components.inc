// Part of libfedrann_hip.so (included by fedrann_hip.hip, behind graph_symmetrize.inc).
//
// fdr_graph_components: which rows of a neighbour graph hang together.  The reference has no counterpart: it writes the
// directed pairs (__main__.py get_output_dataframe) and stops.  For a graph G (ragged rows, as graph_symmetrize.inc
// takes them), a mode m in {union, mutual} and a bound B, the components are the connected components of the undirected
// graph on the n rows in which r != s are joined iff symmetrize_rows(G, m) has the entry (r, s) with distance bits
// <= bits(B):
//     union   an entry (q -> t) with bits <= bits(B) joins q and t;
//     mutual  q and t are joined iff each lists the other and min(b(q->t), b(t->q)) <= bits(B);
// a self entry joins nothing, the bound is inclusive and compares bit patterns.  label[r] in [0, C) numbers the
// components in ascending order of their smallest row, size[c] counts component c's rows: a function of the edge set
// alone.  fedrann_amd.graph.component_labels is the model of this file and the route without a GPU.
//
// C0  The symmetrise's front (gs_rows_by_index): the upload, G1 (the entry's row, the index and distance rules, the
//     packed key) and the segmented sort that orders every row by index, into GraphSymScratch's input arrays.  The held
//     symmetrised graph (gs.rr) is not touched.
// C1  gc_link_kernel<MODE>, one thread per entry (q -> t) of the by-index copy: the repeated-index rule (one comparison
//     with the entry before it in the row); in mutual mode the reverse search (gs_reverse_bits); the bits test; then
//     hook(q, t) on `parent` (int32 [n], the identity at the start).  A hook finds both roots and atomicCASes the larger
//     root's parent from itself to the smaller root; when the CAS loses it goes on from the value the CAS returned.
// C2  gc_flatten_kernel, one thread per row: the walk to the root, root[r], the flag root[r] == r, and count[root[r]]
//     += 1 by integer atomics (order-free).  The lanes of a wave whose root is that of the wave's first live lane add
//     once, their number found by one ballot; the others add singly.  One giant component therefore costs n / 64
//     atomics to one word, not n (returning atomics to one word saturate near 88 per microsecond; these return nothing,
//     but they queue at the same word).
// C3  rocprim::exclusive_scan of the flags: rank[r] is the number of roots below r, rank[n] is C.  gc_label_kernel:
//     label[r] = rank[root[r]], and for a root size[rank[r]] = count[r].
//
// The union-find's invariants:
//  1. parent[x] <= x at all times.  Every walk strictly descends and ends, and a finished component's root is its
//     smallest row.
//  2. A successful CAS only ever changes a root (it expects parent[hi] == hi), and at most n - 1 succeed in total.
//  3. No thread ever waits for another thread's progress: no spin on a flag, no lock.  A hook retries only because
//     some other hook's CAS has succeeded, so by 2 a hook retries fewer than n times.
//  4. Path shortening only ever replaces a parent by one of its ancestors (atomicMin of the grandparent: once y is an
//     ancestor of x it stays one, and of two ancestors the smaller is the farther).  Walks read `parent` by relaxed
//     agent-scope atomic loads, so the compiler keeps none of it in a register across iterations.
// The hub needs no path of its own: a row listed by 20 000 rows costs one successful CAS per distinct root that reaches
// it, and the other hooks are walks that find equal roots.
//
// Device bytes: 28 per entry (GraphSymScratch: index 4, distance 4, row 4, packed key 8, ordered key 8) and 40 per row
// (the indptr 8; parent, root, count, flag, rank, label 4 each; size 8).
// Bounds: as in graph_symmetrize.inc, the host has checked the indptr before the upload.  C1 runs before the host has
// read the refusal record, so it uses t only when 0 <= t < n, whatever the entry holds; parent, root and rank hold
// values of [0, n) only (a parent is a row or was a row's root), count and size are indexed by them.

__device__ __forceinline__ int gc_load(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x's root as it stands; every row passed on the way is given its grandparent
__device__ __forceinline__ int gc_find(int *__restrict__ parent, int x) {
    int p = gc_load(&parent[x]);
    while (p != x) {
        const int g = gc_load(&parent[p]);
        if (g != p) atomicMin(&parent[x], g);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void gc_hook(int *__restrict__ parent, int a, int b) {
    for (;;) {
        a = gc_find(parent, a);
        b = gc_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int was = atomicCAS(&parent[hi], hi, lo);
        if (was == hi) return;
        a = was;  // (another hook has put hi under `was` < hi: hi's component is reached from there)
        b = lo;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void gc_link_kernel(long long total, long long n, unsigned bound,
                                                      const long long *__restrict__ indptr, const int *__restrict__ row,
                                                      const u64 *__restrict__ byidx, int *__restrict__ parent,
                                                      u64 *__restrict__ refusal) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    u64 bad = TM_NONE;
    int q = 0, t = -1;  // the pair to join, where there is one
    if (i < total) {
        q = row[i];
        const u64 key = byidx[i];
        const unsigned listed = (unsigned)(key >> 32);
        unsigned bits = (unsigned)key;
        if (i > indptr[q] && (unsigned)(byidx[i - 1] >> 32) == listed) bad = ((u64)q << 8) | (u64)GS_RULE_REPEAT;
        if ((long long)listed < n && (int)listed != q) {  // (G1 refuses an index outside the rows; here the test keeps t inside)
            bool join = true;
            if (MODE == FDR_GRAPH_MUTUAL) {
                const unsigned back = gs_reverse_bits(indptr, byidx, (long long)listed, q);
                join = back != GS_NO_PARTNER;
                if (back < bits) bits = back;
            }
            if (join && bits <= bound) t = (int)listed;
        }
    }
    gs_refuse(bad, refusal);
    if (t >= 0) gc_hook(parent, q, t);
}

__global__ __launch_bounds__(256) void gc_identity_kernel(long long n, int *__restrict__ parent) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < n) parent[r] = (int)r;
}

// one thread per element of flag: n rows and the 0 behind them
__global__ __launch_bounds__(256) void gc_flatten_kernel(long long n, int *__restrict__ parent, int *__restrict__ root,
                                                         int *__restrict__ flag, unsigned *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = r < n;
    int top = -1;
    if (live) {
        top = gc_find(parent, (int)r);
        root[r] = top;
        flag[r] = top == (int)r;
    } else if (r == n) {
        flag[r] = 0;
    }
    const u64 alive = __ballot(live);
    if (!alive) return;
    const int first = __ffsll((long long)alive) - 1;
    const int lead = __shfl(top, first, 64);
    const bool with = live && top == lead;
    const u64 same = __ballot(with);
    if (with) {
        if (lane == first) atomicAdd(&count[lead], (unsigned)__popcll(same));
    } else if (live) {
        atomicAdd(&count[top], 1u);
    }
}

__global__ __launch_bounds__(256) void gc_label_kernel(long long n, const int *__restrict__ root,
                                                       const int *__restrict__ rank, const unsigned *__restrict__ count,
                                                       int *__restrict__ label, long long *__restrict__ size) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int top = root[r];
    label[r] = rank[top];
    if (top == (int)r) size[rank[r]] = (long long)count[r];
}

FDR_EXPORT int fdr_graph_components(fdr_ctx *ctx, int32_t mode, int64_t n, const int64_t *indptr, const int32_t *idx,
                                    const float *dist, float max_distance, int32_t *label_out, int64_t *size_out,
                                    int64_t *n_components_out) {
    static const char who[] = "graph_components";
    int rc = use_device(ctx);
    if (rc) return rc;
    if (mode != FDR_GRAPH_UNION && mode != FDR_GRAPH_MUTUAL)
        return fail(FDR_E_ARG, "%s: mode %d is neither FDR_GRAPH_UNION nor FDR_GRAPH_MUTUAL (the components of the "
                    "transposed rows are the union's)", who, mode);
    if (n < 1 || n > INT32_MAX) return fail(FDR_E_ARG, "%s: n (%lld) must be in [1, 2^31)", who, (long long)n);
    unsigned bound;
    static_assert(sizeof(bound) == sizeof(max_distance), "a float32's bits");
    memcpy(&bound, &max_distance, sizeof(bound));
    if (bound > 0x7f800000u)
        return fail(FDR_E_ARG, "%s: max_distance is negative or NaN (its bits, 0x%08x, must be at most 0x7f800000)", who,
                    bound);
    if (!indptr || !label_out || !n_components_out) return fail(FDR_E_ARG, "%s: null pointer", who);
    if ((rc = gs_check_indptr(who, n, indptr))) return rc;
    const long long total = indptr[n];
    if (total == 0) {  // (no entries: every row is a component; nothing is uploaded)
        for (int64_t r = 0; r < n; ++r) label_out[r] = (int32_t)r;
        if (size_out)
            for (int64_t r = 0; r < n; ++r) size_out[r] = 1;
        *n_components_out = n;
        return FDR_OK;
    }
    if (!idx || !dist) return fail(FDR_E_ARG, "%s: null pointer", who);
    const hipStream_t st = ctx->stream;
    GraphSymScratch &gs = ctx->gs;
    GraphCompScratch &gc = ctx->gc;
    const size_t rows = (size_t)n;
    if ((rc = gc.parent.reserve(rows))) return rc;
    if ((rc = gc.root.reserve(rows))) return rc;
    if ((rc = gc.count.reserve(rows))) return rc;
    if ((rc = gc.flag.reserve(rows + 1))) return rc;
    if ((rc = gc.rank.reserve(rows + 1))) return rc;
    if ((rc = gc.label.reserve(rows))) return rc;
    if ((rc = gc.size.reserve(rows))) return rc;
    // C0
    if ((rc = gs_rows_by_index(st, gs, n, total, indptr, idx, dist))) return rc;
    const dim3 grid((unsigned)((total + 255) / 256)), per_row((unsigned)((n + 255) / 256)), per_flag((unsigned)(n / 256 + 1)),
        block(256);
    // C1
    hipLaunchKernelGGL(gc_identity_kernel, per_row, block, 0, st, (long long)n, gc.parent.ptr());
    HIP_TRY(hipGetLastError());
    if (mode == FDR_GRAPH_UNION)
        hipLaunchKernelGGL(gc_link_kernel<FDR_GRAPH_UNION>, grid, block, 0, st, total, (long long)n, bound, gs.indptr.ptr(),
                           gs.row.ptr(), gs.byidx.ptr(), gc.parent.ptr(), gs.refusal.ptr());
    else
        hipLaunchKernelGGL(gc_link_kernel<FDR_GRAPH_MUTUAL>, grid, block, 0, st, total, (long long)n, bound, gs.indptr.ptr(),
                           gs.row.ptr(), gs.byidx.ptr(), gc.parent.ptr(), gs.refusal.ptr());
    HIP_TRY(hipGetLastError());
    // C2, C3  (on a refused graph too: every parent is a row, and the host reads the record before any output)
    HIP_TRY(hipMemsetAsync(gc.count.ptr(), 0, rows * sizeof(unsigned), st));
    hipLaunchKernelGGL(gc_flatten_kernel, per_flag, block, 0, st, (long long)n, gc.parent.ptr(), gc.root.ptr(),
                       gc.flag.ptr(), gc.count.ptr());
    HIP_TRY(hipGetLastError());
    auto scan = [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, gc.flag.ptr(), gc.rank.ptr(), 0, rows + 1, rocprim::plus<int>(), st);
    };
    if ((rc = rocprim_run(gs.tmp, "rocprim::exclusive_scan", scan))) return rc;
    hipLaunchKernelGGL(gc_label_kernel, per_row, block, 0, st, (long long)n, gc.root.ptr(), gc.rank.ptr(), gc.count.ptr(),
                       gc.label.ptr(), gc.size.ptr());
    HIP_TRY(hipGetLastError());
    u64 refused = TM_NONE;
    int found = 0;
    HIP_TRY(download(&refused, gs.refusal, 1, st));
    HIP_TRY(hipMemcpyAsync(&found, gc.rank.ptr() + rows, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (refused != TM_NONE) return gs_refused(who, refused);  // (nothing has been written to the outputs)
    if (found < 1 || (long long)found > (long long)n)
        return fail(FDR_E_HIP, "internal: %s: %d components of %lld rows", who, found, (long long)n);
    static_assert(sizeof(int) == sizeof(int32_t), "the caller's labels are the device's");
    HIP_TRY(download(reinterpret_cast<int *>(label_out), gc.label, rows, st));
    if (size_out) HIP_TRY(download(reinterpret_cast<long long *>(size_out), gc.size, (size_t)found, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_components_out = found;
    return FDR_OK;
}
