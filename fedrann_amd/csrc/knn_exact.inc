// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit), not compiled on its own.
// ------------------------------------------------------------------------------------------
// K3  tiled exact cosine k-NN.
//
// Workgroup = 8 waves = 256 query rows; grid = (query blocks, target segments).  Each wave keeps
// its 32 queries as the B operand of v_mfma_f32_32x32x2_f32 in DP/2 VGPRs for the whole kernel
// and streams 32-target tiles (A operand) from a double-buffered, XOR-swizzled LDS image shared by
// the 8 waves.  The MFMA accumulates along K exactly like an fp32 fmaf chain in ascending
// component order, so every similarity is bit-identical to the CPU oracle's chain_dot().
//
// Top-k: one list of K (dist,idx) keys per query in LDS (key = dist bits << 32 | idx, unsigned
// order == (dist asc, idx asc)); the list is an unsorted set whose maximum (tau, taupos) is kept
// in registers.  Fast path per tile: max of the 16 accumulators -> one distance -> compare with
// tau.  Slow path (rare after warm-up): candidates are visited in ascending target order --
// lane-half 0 takes tile rows 0..15, then lane-half 1 rows 16..31 -- so a strict "dist < tau" is
// exact under the (dist, idx) order; an accepted candidate replaces the maximum and the K keys
// are rescanned for the new maximum.
// ------------------------------------------------------------------------------------------
#define KEY_INF 0x7F800000FFFFFFFFull

__device__ __forceinline__ float dist_from_sim(float c) {
    return __builtin_amdgcn_fmed3f(1.0f - c, 0.0f, 1.0f);  // clamp(1 - c, 0, 1): v_sub + v_med3
}

// Conservative similarity-space form of "dist_from_sim(c) < tau": every c that passes the exact
// test satisfies c > sim_floor(tau) (both roundings involved are below 6e-8 in [0,1]); candidates
// above the floor are re-tested exactly before they are queued.
__device__ __forceinline__ float sim_floor(float tau) {
    return tau <= 1.0f ? (1.0f - tau) - 3.0e-7f : -__builtin_inff();
}

// zero-row byte flags -> one bit per target row (bit r of word w = row 32w + r)
__global__ __launch_bounds__(256) void pack_zero_bits_kernel(const unsigned char *__restrict__ zero,
                                                             int n, unsigned *__restrict__ bits,
                                                             unsigned *__restrict__ tau_shared,
                                                             int n_shared) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_shared; i += gridDim.x * 256)
        tau_shared[i] = 0x7F800000u;  // +inf: no segment has a full list yet
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool z = i < n && zero[i] != 0;
    const u64 m = __ballot(z);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && i < n) bits[i >> 5] = (unsigned)m;
    if (lane == 32 && i < n) bits[i >> 5] = (unsigned)(m >> 32);
}

// ---- top-k state of one 32-query set of a wave ---------------------------------------------------
// A query (lane pair j / j+32) owns one unsorted list of K keys in LDS (column `ql` of lists[K][256]);
// taukey / taupos = its current maximum, identical in both lanes.  Each LANE additionally owns a
// 4-entry append queue in LDS.  Per tile, candidates that beat tau (which may be stale, i.e. too
// large, between flushes -- that only admits extra candidates) are appended to the lane's queue with
// predicated stores; when a queue overflows, and at the end of the segment, the whole wave flushes:
// every queued key that is still smaller than the list maximum replaces it and the two lanes of the
// query rescan the list together.  Exactness: keys order by (dist, idx); a rejected candidate has
// dist >= tau.dist and a larger index than every listed key, so it can never belong to the top-k.
// (QCAP, FDR_MAX_SEG and SegBounds: knn_plan.inc)

// Development builds (-DFDR_DEV, devtools/build_dev.sh) give the search kernels a `dbg` argument fed from
// FDR_KNN_DEBUG (bit 0: skip the top-k slow path -- WRONG RESULTS, timing experiments only; bit 1: event
// counters with -DFDR_DEBUG_COUNTERS; bit 2: no bound refresh; bit 3: print the plan).  The release library
// has neither the argument nor the code behind it.
#ifdef FDR_DEV
#define FDR_DBG_PARAM , int dbg
#define FDR_DBG_ARG(x) , (x)
#else
#define FDR_DBG_PARAM
#define FDR_DBG_ARG(x)
#endif
#ifdef FDR_DEBUG_COUNTERS  // development build only: event counters read back with FDR_KNN_DEBUG=2
__device__ unsigned long long g_dbg_counters[8];
#define DBG_COUNT(i) do { if (dbgc && (threadIdx.x & 63) == 0) atomicAdd(&g_dbg_counters[i], 1ull); } while (0)
#define DBG_ADD(i, n) do { if (dbgc && (threadIdx.x & 63) == 0) atomicAdd(&g_dbg_counters[i], (unsigned long long)(n)); } while (0)
#else
#define DBG_COUNT(i) do { (void)dbgc; } while (0)
#define DBG_ADD(i, n) do { (void)dbgc; } while (0)
#endif

struct TopkState {
    u64 taukey;   // maximum key of the query's list (both lanes of the query hold the same value)
    float tau;    // admission bound: min(distance part of taukey, cross-segment bound), see topk_share
    float cfloor; // sim_floor(tau)
    int taupos;   // position of taukey in the list
    int qcnt;     // entries in this LANE's append queue
    float foreign;  // last cross-segment bound seen (strict form, +inf if none): see topk_share
};

// Cross-segment bound.  Workgroups that search different target segments for the same queries
// publish the k-th best distance of their (full) list with a relaxed device-scope atomicMin on one
// word per query and adopt the minimum any segment has published.  Every published value is an upper
// bound of the query's final k-th best distance D, so a candidate with dist > bound can never be in
// the final top-k; candidates with dist == bound are kept (ties are decided by index in the merge):
// the admission test is dist < nextup(bound).  A stale or missing value only admits more candidates,
// so the result does not depend on scheduling, timing or placement.
__device__ __forceinline__ float topk_share(unsigned *__restrict__ slot, const u64 taukey, const int h,
                                            float &foreign_out) {
    const unsigned mine = (unsigned)(taukey >> 32);  // 0x7F800000 while the list still has empty slots
    unsigned seen = mine;
    if (h == 0) {
        const unsigned old = mine < 0x7F800000u
                                 ? __hip_atomic_fetch_min(slot, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                 : __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        seen = old < mine ? old : mine;
    }
    seen = __shfl(seen, (threadIdx.x & 31), 64) ;  // lane j (h == 0) of this query holds the value
    // strict bound: the list's own maximum admits dist < tau; a foreign bound admits dist <= bound
    const float own = __uint_as_float(mine);
    const float foreign = seen < 0x7F800000u ? __uint_as_float(seen + 1u) : __builtin_inff();
    foreign_out = foreign;
    return fminf(own, foreign);
}

template <int NT, int QW>
__device__ __noinline__ TopkState topk_flush(TopkState st, u64 *__restrict__ lists,
                                             u64 *__restrict__ queue, unsigned *__restrict__ shared,
                                             const int ql, const int K, const int tid, const int h,
                                             const int qcap, const bool dbgc) {
    DBG_COUNT(2);
    const int cnt_me = st.qcnt;
    const int cnt_other = __shfl_xor(cnt_me, 32);
#pragma unroll 1
    for (int ph = 0; ph < 2; ++ph) {
        const int owner_cnt = (h == ph) ? cnt_me : cnt_other;
        const int owner_tid = (tid & ~32) | (ph << 5);
#pragma unroll 1
        for (int i = 0; i < qcap; ++i) {
            const bool active = i < owner_cnt;
            if (!__any(active)) break;
            u64 key = KEY_INF;
            if (active) key = queue[i * NT + owner_tid];
            const bool ins = active && key < st.taukey;
            DBG_COUNT(3);
            if (__any(ins)) {
                DBG_COUNT(4);
                if (ins) {
                    if (h == 0) lists[st.taupos * QW + ql] = key;
                    // both lanes of the query rescan the list: lane-half h takes entries h, h+2, ...
                    u64 best = 0;
                    int bp = 0;
#pragma unroll 2
                    for (int e = h; e < K; e += 2) {
                        const u64 kv = lists[e * QW + ql];
                        if (kv > best) {
                            best = kv;
                            bp = e;
                        }
                    }
                    const u64 ob = __shfl_xor(best, 32);
                    const int op = __shfl_xor(bp, 32);
                    if (ob > best) {
                        best = ob;
                        bp = op;
                    }
                    st.taukey = best;
                    st.taupos = bp;
                }
            }
        }
    }
    // (no atomic here: a flush must not wait for a global round trip; the bound is exchanged by the
    // periodic topk_share calls of the tile loop)
    st.tau = fminf(__uint_as_float((unsigned)(st.taukey >> 32)), st.foreign);
    st.cfloor = sim_floor(st.tau);
    st.qcnt = 0;
    return st;
}

// Queue every candidate of this tile that beats tau.  acc[r] = similarity of query j with tile row
// (r&3) + 8*(r>>2) + 4*h; rows >= nvalid do not exist (last tile of a segment only).
template <int NT, int QW>
__device__ __forceinline__ void topk_append(const f32x16 acc, TopkState &st, u64 *__restrict__ lists,
                                            u64 *__restrict__ queue, unsigned *__restrict__ shared,
                                            const int ql, const int K, const int tid, const int h,
                                            int idx0, int nvalid, const int qcap, const bool dbgc) {
    // this block is cold: keep its address / index arithmetic from being hoisted into the hot loop
    asm volatile("" : "+s"(idx0), "+s"(nvalid));
    unsigned todo = 0xffffu;
    if (nvalid < 32) {
        todo = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            todo |= ((r & 3) + 8 * (r >> 2) + 4 * h < nvalid) ? (1u << r) : 0u;
    }
    const int idxh = idx0 + 4 * h;
    // First pass over a tile: "dist < tau" is exact, because every listed or queued key comes from an
    // earlier tile (smaller index).  After a mid-tile flush the list may hold rows of THIS tile from
    // the partner lane, whose indices interleave with mine, so a retried candidate with dist == tau
    // can still win on the index: retries admit dist <= tau and the flush's full-key test decides.
    bool retry = false;
#pragma unroll 1
    while (true) {
        DBG_COUNT(1);
        unsigned ovf = 0;
        // (a retry admits dist == tau; on the clamp plateau tau == 1 that is EVERY similarity <= 0, which the
        // similarity-space gate sim_floor(1) = -3e-7 would cut off: no gate there)
        const float gate = (retry && st.tau >= 1.0f) ? -__builtin_inff() : st.cfloor;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (acc[r] > gate) {
                // everything below is kept inside this (rarely taken) block: the asm makes the
                // candidate opaque so that hipcc cannot evaluate the block's arithmetic eagerly
                float a = acc[r];
                asm volatile("" : "+v"(a));
                const float dist = dist_from_sim(a);
                if (((todo >> r) & 1u) && (dist < st.tau || (retry && dist == st.tau))) {
                    if (st.qcnt < qcap) {
                        queue[st.qcnt * NT + tid] =
                            ((u64)__float_as_uint(dist) << 32) | (unsigned)(idxh + (r & 3) + 8 * (r >> 2));
                        ++st.qcnt;
                    } else {
                        ovf |= 1u << r;
                    }
                }
            }
        }
        if (!__any(ovf != 0u)) break;
        st = topk_flush<NT, QW>(st, lists, queue, shared, ql, K, tid, h, qcap, dbgc);
        todo = ovf;
        retry = true;
    }
}

// DP: padded embedding length.  NQ: 32-query sets per wave (independent MFMA accumulator chains
// that share every A fragment).  NW: waves per workgroup; a workgroup owns QW = 32*NQ*NW queries.
// WPS: waves per SIMD the register budget is sized for.
// LDS: 2-stage ring of 32 target rows x 64 components (16 KB) | lists K x QW keys | queues.
template <int DP, int NQ, int NW, int WPS>
__global__ __launch_bounds__(64 * NW, WPS) void knn_tile_kernel(
    const float *__restrict__ Qh, const unsigned char *__restrict__ qzero, int nq,
    const float *__restrict__ Th, const unsigned *__restrict__ tzbits, int nt, int t_base,
    SegBounds segs, int K, int nq_pad, u64 *__restrict__ partial, unsigned *__restrict__ tau_shared,
    int qcap, int item_base, int nqb FDR_DBG_PARAM) {
#ifndef FDR_DEV
    constexpr int dbg = 0;
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // work item = (target segment, query block), segment-major; a launch covers the items item_base .. of a
    // one-dimensional grid (launch_knn_exact: one launch, or synchronised rounds of at most one workgroup per slot)
    const int item = item_base + (int)blockIdx.x;
    const int seg = item / nqb, qb = item - seg * nqb;
    constexpr int NT = 64 * NW;              // threads per workgroup
    constexpr int QW = 32 * NQ * NW;         // queries per workgroup
    constexpr int NCH = DP / 64;             // 64-component K-chunks per tile
    constexpr int STAGE_BYTES = 32 * 64 * 4; // one stage = 32 target rows x 64 components (8 KB)
    constexpr int SLOTS = 16;                // 16-byte slots per staged row
    constexpr int NSTAGE = 2;                // LDS ring: stage it lives in buffer it % 2
    u64 *lists = reinterpret_cast<u64 *>(smem + NSTAGE * STAGE_BYTES);                         // K * QW keys
    u64 *queues = reinterpret_cast<u64 *>(smem + NSTAGE * STAGE_BYTES + (size_t)K * QW * 8);  // NQ*QCAP*NT

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;

    // queries: this lane's B fragments for all DP/2 K-steps of each of its NQ query sets
    float b[NQ][DP / 2];
    bool qz[NQ];
    int ql[NQ];
    int qslot[NQ];  // index of this query's cross-segment bound word
    bool any_qz = false;
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
        ql[s] = (wave * NQ + s) * 32 + j;
        const int qg = qb * QW + ql[s];
        qslot[s] = qg;
        const int qrow = qg < nq ? qg : nq - 1;
        qz[s] = qzero[qrow] != 0;
        any_qz = any_qz || __any(qz[s]);
        const f32x4 *qp = reinterpret_cast<const f32x4 *>(Qh + (size_t)qrow * DP);
#pragma unroll
        for (int g = 0; g < DP / 8; ++g) {
            const f32x4 v = qp[2 * g + h];
            b[s][4 * g + 0] = v.x;
            b[s][4 * g + 1] = v.y;
            b[s][4 * g + 2] = v.z;
            b[s][4 * g + 3] = v.w;
        }
    }
    for (int i = tid; i < K * QW; i += NT) lists[i] = KEY_INF;
    TopkState st[NQ];
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
        st[s].taukey = KEY_INF;
        st[s].taupos = 0;
        st[s].qcnt = 0;
        st[s].tau = topk_share((tau_shared + qslot[s]), KEY_INF, h, st[s].foreign);  // other segments may already have a bound
        st[s].cfloor = sim_floor(st[s].tau);
    }

    const int t_begin = segs.b[seg];  // multiple of 32
    const int t_end = min(nt, segs.b[seg + 1]);
    const int ntiles = (t_end - t_begin + 31) >> 5;
    const int nstages = ntiles * NCH;

    // staging by LDS-DMA (global_load_lds_dwordx4): each wave-instruction fills 1 KiB = four staged
    // rows of 256 B, linearly; the XOR swizzle that makes the MFMA loop's ds_read_b128 (32 rows x one
    // slot) bank-conflict free is applied to the SOURCE slot instead.  Rows past the segment end
    // re-read the last valid row (finite garbage; such candidates are masked by nvalid).
    constexpr int NPIECE = 8;  // 1 KiB pieces per stage, dealt round-robin to the waves
    auto issue_stage = [&](int it, int buf) {
        const int t = it / NCH, ch = it % NCH;
        const int trow0 = t_begin + t * 32;
#pragma unroll
        for (int u = 0; u < (NPIECE + NW - 1) / NW; ++u) {
            const int piece = wave + NW * u;
            if (NPIECE % NW != 0 && piece >= NPIECE) break;
            const int row = 4 * piece + (lane >> 4), pslot = lane & 15;
            const int trow = min(trow0 + row, t_end - 1);
            const float *src = Th + (size_t)trow * DP + (size_t)(ch * SLOTS + (pslot ^ (row & 15))) * 4;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)src,
                (__attribute__((address_space(3))) void *)(smem + buf * STAGE_BYTES + piece * 1024), 16, 0, 0);
        }
    };

    // Two-stage ring: stage it+1 is issued at the top of iteration it and must have landed by the
    // barrier at its bottom (hipcc drains vmcnt before __syncthreads()).  A three-stage ring with a
    // counted vmcnt and a raw s_barrier was measured and bought nothing here (three waves per SIMD
    // already hide the DMA latency), so the simpler form stays.
    if (nstages > 0) issue_stage(0, 0);
    __syncthreads();  // also publishes the list initialisation

    for (int t = 0; t < ntiles; ++t) {
        f32x16 acc[NQ];
#pragma unroll
        for (int s = 0; s < NQ; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int it = t * NCH + ch;
            const int buf = it % NSTAGE;
            if (it + 1 < nstages) issue_stage(it + 1, (it + 1) % NSTAGE);

            // ---- 32 targets x (NQ x 32) queries x 64 components ----
            {
                const f32x4 *sb = reinterpret_cast<const f32x4 *>(smem + buf * STAGE_BYTES) + j * SLOTS;
                const int sw = j & 15;
                f32x4 a[3];  // fragment ring: two groups prefetched ahead of the MFMAs
                a[0] = sb[(0 + h) ^ sw];
                a[1] = sb[(2 + h) ^ sw];
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    if (g + 2 < 8) a[(g + 2) % 3] = sb[(2 * (g + 2) + h) ^ sw];
                    const f32x4 av = a[g % 3];
                    const int bb = 32 * ch + 4 * g;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int s = 0; s < NQ; ++s)
                            acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b[s][bb + e], acc[s], 0, 0, 0);
                }
            }

            if (ch == NCH - 1) {
                const int tile_row0 = t_begin + t * 32;
                if (any_qz) {  // rare: an all-zero query is at distance 0 from all-zero targets, 1 from the rest
                    const unsigned zm = tzbits[(t_begin >> 5) + t] >> (4 * h);  // wave-uniform load
#pragma unroll
                    for (int s = 0; s < NQ; ++s)
                        if (qz[s]) {
#pragma unroll
                            for (int r = 0; r < 16; ++r)
                                acc[s][r] = (float)((zm >> ((r & 3) + 8 * (r >> 2))) & 1u);
                        }
                }
#pragma unroll
                for (int s = 0; s < NQ; ++s) {
                    // fast path: can any of my 16 candidates beat the current k-th best?
                    float mx = acc[s][0];
#pragma unroll
                    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[s][r]);
                    if (dbg & 1) {  // timing experiment: MFMA + fast path only
                        if (mx > 3.0e38f) st[s].tau = mx;
                        continue;
                    }
                    if (__any(mx > st[s].cfloor))
                        topk_append<NT, QW>(acc[s], st[s], lists, queues + s * qcap * NT, (tau_shared + qslot[s]), ql[s],
                                            K, tid, h, t_base + tile_row0, t_end - tile_row0, qcap, (dbg & 2) != 0);
                    if ((t & 31) == 31 && !(dbg & 4)) {  // refresh the cross-segment bound now and then
                        st[s].tau = topk_share((tau_shared + qslot[s]), st[s].taukey, h, st[s].foreign);
                        st[s].cfloor = sim_floor(st[s].tau);
                    }
                }
            }
            __syncthreads();  // stage it+1 is complete (every wave's pieces) before anyone reads it
        }
    }

    // ---- drain the queues, then write this segment's lists: partial[seg][query][K] ----
#pragma unroll
    for (int s = 0; s < NQ; ++s)
        if (__any(st[s].qcnt > 0))
            st[s] = topk_flush<NT, QW>(st[s], lists, queues + s * qcap * NT, (tau_shared + qslot[s]), ql[s], K, tid, h,
                                       qcap, (dbg & 2) != 0);
    __syncthreads();
    {
        u64 *out = partial + ((size_t)seg * nq_pad + (size_t)qb * QW) * K;
        const int total = QW * K;
        for (int i = tid; i < total; i += NT) {
            const int q = i / K, e = i % K;
            out[i] = lists[e * QW + q];
        }
    }
}

// ------------------------------------------------------------------------------------------
// K4  merge: one wave per query selects the K smallest keys out of nseg * K, ascending.
// Keys are unique (each target lives in exactly one segment), so "smallest key greater than the
// previous pick" enumerates them in order.
// ------------------------------------------------------------------------------------------
#define MERGE_CAP 512  // keys per query staged in LDS; longer candidate sets are re-read from global

// PICKS: picks per lane (K <= 64 * PICKS); stage: this wave's CAP keys of LDS
template <int PICKS, int CAP>
__device__ __forceinline__ void knn_merge_query(const u64 *__restrict__ partial, int nseg, int q, int nq_pad, int K,
                                                u64 *mine_lds, int *__restrict__ idx_out, float *__restrict__ dist_out) {
    const int lane = threadIdx.x & 63;
    const int M = nseg * K;
    const bool staged = M <= CAP;
    if (staged) {  // one pass over global memory; the k selection rounds then run out of LDS
        for (int m = lane; m < M; m += 64) {
            const int seg = m / K, e = m - seg * K;
            mine_lds[m] = partial[((size_t)seg * nq_pad + q) * K + e];
        }
    }
    u64 prev1 = 0;  // previous pick + 1 (0 = none yet)
    u64 mine = 0, mine1 = 0;  // picks lane and (PICKS = 2) lane + 64
    for (int r = 0; r < K; ++r) {
        u64 best = ~0ull;
        for (int m = lane; m < M; m += 64) {
            u64 kv;
            if (staged) {
                kv = mine_lds[m];
            } else {
                const int seg = m / K, e = m - seg * K;
                kv = partial[((size_t)seg * nq_pad + q) * K + e];
            }
            if (kv + 1 > prev1 && kv < best) best = kv;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(best, off);
            best = o < best ? o : best;
        }
        prev1 = best + 1;
        if (lane == r) mine = best;
        if (PICKS > 1 && lane + 64 == r) mine1 = best;
    }
    if (lane < K) {
        idx_out[(size_t)q * K + lane] = (int)(unsigned)(mine & 0xffffffffull);
        dist_out[(size_t)q * K + lane] = __uint_as_float((unsigned)(mine >> 32));
    }
    if (PICKS > 1 && lane + 64 < K) {
        idx_out[(size_t)q * K + lane + 64] = (int)(unsigned)(mine1 & 0xffffffffull);
        dist_out[(size_t)q * K + lane + 64] = __uint_as_float((unsigned)(mine1 >> 32));
    }
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const u64 *__restrict__ partial, int nseg,
                                                        int nq, int nq_pad, int K,
                                                        int *__restrict__ idx_out,
                                                        float *__restrict__ dist_out) {
    __shared__ u64 stage[4][MERGE_CAP];
    const int wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    if (q >= nq) return;
    knn_merge_query<1, MERGE_CAP>(partial, nseg, q, nq_pad, K, stage[wave], idx_out, dist_out);
}

// K4w  merge for 64 < K <= FDR_EXACT_MAX_K: two picks per lane (lane l keeps picks l and l + 64); the planner keeps
// nseg * K <= FDR_MERGE_WIDE_CAP (knn_plan_compute), so every query's keys are staged in LDS.
__global__ __launch_bounds__(256) void knn_merge_wide_kernel(const u64 *__restrict__ partial, int nseg,
                                                             int nq, int nq_pad, int K,
                                                             int *__restrict__ idx_out,
                                                             float *__restrict__ dist_out) {
    __shared__ u64 stage[4][FDR_MERGE_WIDE_CAP];
    const int wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    if (q >= nq) return;
    knn_merge_query<2, FDR_MERGE_WIDE_CAP>(partial, nseg, q, nq_pad, K, stage[wave], idx_out, dist_out);
}
