// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit), not compiled on its own.
// ------------------------------------------------------------------------------------------
// Half-precision prefilter (the default mode whenever k + 8 <= 64 and the lists fit in LDS).
//
// P1 knn_prefilter_kernel: the same tiling and top-k machinery as K3, but the similarities come
//    from v_mfma_f32_32x32x16_f16 on fp16 copies of the normalised rows (16x the fp32 MFMA rate)
//    and the lists keep K' = K + 8 candidates per query, ordered by the APPROXIMATE distance.
// P2 knn_rerank_kernel: per query, certifies that the K' candidates contain the exact top-K and, if
//    so, recomputes their distances with the canonical fp32 fma chain and selects the K best by
//    (dist, idx); otherwise the query is queued for the exact kernel (K3).
//
// Certificate.  Let eps bound |s~ - c| over all pairs (fp16 rounding of unit rows: 2*2^-11 relative
// on sum |x||y| <= 1, plus subnormal and fp32 accumulation terms; FDR_PREFILTER_EPS), d~ the
// approximate distances, d~(K) and d~(K') the K-th and K'-th smallest.  If
//        d~(K) + M < 1   and   d~(K) + M < d~(K'),      M = 2*eps + 4e-7,
// then every target outside the list has d~ >= d~(K') > d~(K) + M, hence an exact distance larger
// than d~(K) + eps + 4e-7, while the K list members with the smallest d~ have exact distances
// <= d~(K) + eps: nothing outside the list can reach the exact top-K, not even through an fp32
// rounding tie (the 4e-7), and "< 1" keeps the argument inside the region where the distance is
// strictly monotone in the similarity (no clamp plateau).  All-zero queries (d~ = 1 everywhere) and
// heavy near-tie plateaus fail the test and take the exact path, so the final result is always the
// canonical one.
// ------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// (FDR_PREFILTER_EPS / _EXTRA / _MAX_IB, prefilter_index_bits(), prefilter_eps(), prefilter_extra(): knn_plan.inc)

// Ehat fp32 [n, DP] (k0 k2 k4 k6 k1 k3 k5 k7 inside each group of 8) -> fp16 [n, DP], natural order
// group t of 8 components: v[] = its fp32 values in natural (canonical-chain) order, their fp16 roundings stored
__device__ __forceinline__ void to_half_group(const float *__restrict__ Ehat, long long t, _Float16 *__restrict__ out,
                                              float (&v)[8]) {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(Ehat) + t * 2;
    const f32x4 e = src[0], o = src[1];  // even components k0 k2 k4 k6 | odd components k1 k3 k5 k7
    v[0] = e.x; v[1] = o.x; v[2] = e.y; v[3] = o.y; v[4] = e.z; v[5] = o.z; v[6] = e.w; v[7] = o.w;
    f16x8 h;
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = (_Float16)v[i];
    reinterpret_cast<f16x8 *>(out)[t] = h;
}
__global__ __launch_bounds__(256) void to_half_kernel(const float *__restrict__ Ehat, long long n_groups,
                                                      _Float16 *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;  // one thread per 8 components
    if (t >= n_groups) return;
    float v[8];
    to_half_group(Ehat, t, out, v);
}

// to_half_kernel for rows of RC_DP components that also writes each row's compact record (knn_workspace.inc: RC_*)
// while the row is in registers: the 16 threads of a row are 16 adjacent lanes, a prefix sum over them gives every
// non-zero component (bits & 0x7fffffff != 0: -0.0f is a zero) its entry number in canonical-chain order.  A row with
// more than RC_ENTRIES non-zeros gets its count alone; such rows are counted in *n_long, one atomic per workgroup.
__global__ __launch_bounds__(256) void to_half_compact_kernel(const float *__restrict__ Ehat, long long n_groups,
                                                              _Float16 *__restrict__ out, unsigned char *__restrict__ rc,
                                                              int *__restrict__ n_long) {
    __shared__ int wg_long;
    if (threadIdx.x == 0) wg_long = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < n_groups;  // (n_groups is a multiple of 16: the lanes of a row are live together)
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) to_half_group(Ehat, t, out, v);
    const int g = (int)(t & 15);
    unsigned nzm = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) nzm |= (unsigned)((__float_as_uint(v[i]) & 0x7fffffffu) != 0u) << i;
    const int mine = __popc(nzm);
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const int below = __shfl_up(incl, off, 16);
        if (g >= off) incl += below;
    }
    const int total = __shfl(incl, 15, 16);  // (<= RC_DP: fits the count byte)
    if (live) {
        unsigned char *rec = rc + (size_t)(t >> 4) * RC_BYTES;
        if (g == 0) rec[0] = (unsigned char)total;
        if (total <= RC_ENTRIES) {
            int e = incl - mine;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if ((nzm >> i) & 1u) {
                    unsigned char *hf = rec + 64 * (e / RC_HALF_ENTRIES);
                    const int s = e % RC_HALF_ENTRIES;
                    hf[1 + s] = (unsigned char)(8 * g + (i & 1) * 4 + (i >> 1));  // where component 8 g + i is stored
                    reinterpret_cast<float *>(hf + 16)[s] = v[i];
                    ++e;
                }
            }
        }
    }
    const u64 lm = __ballot(live && g == 0 && total > RC_ENTRIES);
    if ((threadIdx.x & 63) == 0 && lm) atomicAdd(&wg_long, __popcll(lm));
    __syncthreads();
    if (threadIdx.x == 0 && wg_long) atomicAdd(n_long, wg_long);
}

// ds_read_b128 with an immediate offset, outside hipcc's waitcnt bookkeeping (the caller waits with a
// counted s_waitcnt lgkmcnt that names the destination, see the prefilter pass's k-loop)
template <int OFF>
__device__ __forceinline__ void lds_read128(f16x8 &dst, unsigned addr, std::integral_constant<int, OFF>) {
    static_assert(OFF >= 0 && OFF < 65536, "ds_read offset is 16 bits");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}

// s_waitcnt lgkmcnt(N) with a literal count, tied to the fragment register the caller is about to use
template <int N>
__device__ __forceinline__ void wait_lgkmcnt(f16x8 &frag) {
    static_assert(N >= 0 && N <= 6, "count out of range");
    if constexpr (N == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(frag));
    else if constexpr (N == 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(frag));
    else if constexpr (N == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(frag));
    else if constexpr (N == 3) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(frag));
    else if constexpr (N == 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(frag));
    else if constexpr (N == 5) asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(frag));
    else asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(frag));
}

template <int... S, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, S...>, F &&f) {  // f(integral_constant<int, S>{}) for every S
    (f(std::integral_constant<int, S>{}), ...);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {  // s_waitcnt vmcnt(N) with a literal count
    static_assert(N >= 0 && N <= 16, "count out of range");
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else static_assert(N == 0, "add the literal form for this count");
}

// ---- P1 top-k state: 32-bit keys in sorted register lists ------------------------------------
// key = qd << ib | row - segment start.  qd = QM1 - rint(clamp(sim, 0, 1) * QM1) is the approximate
// distance on a grid of QM1 = 2^qbits - 2 steps (qbits = min(20, 32 - ib); ib = bits of the longest
// segment, chosen per launch), so the order of keys is (quantised distance, row).  The grid adds
// 0.5 / QM1 to the prefilter's error bound (see prefilter_eps()).  EMPTY = all ones is larger than any key.
// The K' keys of a query live in REGISTERS: lane j holds LH of them and lane j + 32 the other LH, each
// half sorted ascending (positions beyond K' are pinned to key 0 and skipped at write-out).  The
// list's maximum is therefore max(v[LH-1], partner's v[LH-1]); inserting c means: the half that
// holds the maximum drops it and takes c, one v_med3_u32 per element
//     v'[e] = med3(v[e-1], c, v[e]),  v'[0] = min(v[0], c)
// (inserting EMPTY changes nothing, which is how the other half and idle queries sit the round out).
// A round costs ~LH + 12 VALU instructions for all 32 queries of the wave at once, no LDS and no scan.
#define PK_EMPTY 0xffffffffu
#ifdef FDR_STAMPS  // development (-DFDR_STAMPS): where the waves of workgroup 0 spend a stage (s_memtime deltas, summed per wave)
__device__ unsigned long long g_stamps[16][8];  // [wave][phase]
#define STAMP(v) const unsigned v = (unsigned)__builtin_readcyclecounter()
#define STAMP_ADD(ph, a, b) do { if (stamp_on) stamp_acc[ph] += (b) - (a); } while (0)  // (32-bit sums of 32-bit stamps: few registers)
#else
#define STAMP(v) do { } while (0)
#define STAMP_ADD(ph, a, b) do { } while (0)
#endif
// the lists are flushed and the bounds exchanged every (FDR_SHARE_EVERY + 1) stages (a power of two - 1):
// 16 / 32 / 64 / 128 stages = 96.3 / 95.0 / 94.4 / 94.1 ms at 1 M rows, 8 stages 99.1; flat at 100 k rows
constexpr int FDR_SHARE_EVERY = 63;


// A lane's eight fragment addresses inside a unit of 32 rows x 128 fp16 components: k-step s reads the 16-byte slot
// (2 s + h) ^ (j & 15) of row j (the slots are XOR-swizzled with the row when the LDS-DMA writes them).  They are LDS
// addresses, ring base included, so that a read is `ds_read_b128 v, fa[s] offset:stage/unit`.
__device__ __forceinline__ void fragment_addresses(unsigned (&fa)[8], const unsigned char *ring_base, int j, int h) {
    const unsigned ring = (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char *)ring_base;
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) {
        fa[s8] = ring + (unsigned)(j * 256 + (((2 * s8 + h) ^ (j & 15)) * 16));
        asm volatile("" : "+v"(fa[s8]));  // (opaque: otherwise hipcc re-derives it with a v_add per read)
    }
}

__device__ __forceinline__ unsigned partner32(unsigned x, int h) {  // value held by lane ^ 32
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return h ? r[0] : r[1];
}

template <int LH>
struct RegList {
    unsigned v[LH];
    unsigned pmax;  // partner half's maximum
};

// one insertion round: every query takes the smaller of its two lanes' candidates (PK_EMPTY = none);
// returns the candidate that was considered (the other lane's, if any, must be offered again)
template <int LH>
__device__ __forceinline__ unsigned reglist_round(RegList<LH> &L, unsigned cand, int h) {
    const unsigned c = min(cand, partner32(cand, h));
    const unsigned mymax = L.v[LH - 1];
    const bool hold = mymax > L.pmax || (mymax == L.pmax && h == 0);
    const unsigned ce = (hold && c < mymax) ? c : PK_EMPTY;  // (hold => mymax is the list maximum)
#pragma unroll
    for (int e = LH - 1; e >= 1; --e) L.v[e] = max(min(L.v[e - 1], ce), min(max(L.v[e - 1], ce), L.v[e]));
    L.v[0] = min(L.v[0], ce);
    L.pmax = partner32(L.v[LH - 1], h);
    return c;
}

// Ordered scan (knn_order.inc): Qh / Th are fp16 copies in mask order; the lists go back to the rows' own numbers.
struct OrderArgs {
    const int *perm_t;  // scan position -> target row (null: the rows are scanned as they are)
    const int *perm_q;  // query position -> query row
};

// NW waves with NQ 32-query sets each (QW = 32*NQ*NW queries per workgroup; the NQ accumulator chains
// of a wave share every target fragment read from LDS).  The targets stream through a two-stage LDS
// ring; a stage holds U "units" of 32 rows x 128 fp16 components (8 KB each).  LDS holds nothing else
// (the top-k lists are in registers), so the workgroups per CU are set by the register budget (WPS
// waves per SIMD).
// The loop is bound by VALU ISSUE, not by the MFMA pipe: a tile's 8 MFMAs occupy the pipe for 256
// cycles, and every vector instruction of the SIMD's waves costs 4 issue cycles beside them.  Hence:
// integer max3 tree on the accumulator bits (10 instructions per tile, group maxima as by-products),
// stage parity unrolled so that every ds_read address is a register + immediate, LDS-DMA sources as
// 32-bit offsets advanced by a constant, the wave number in an SGPR.
template <int DP, int NQ, int NW, int WPS, int U, int LH, bool PAIRED = false>
__global__ __launch_bounds__(64 * NW, WPS) void knn_prefilter_kernel(
    const _Float16 *__restrict__ Qh, int nq, const _Float16 *__restrict__ Th, int nt, int t_base,
    SegBounds segs, int K, int nq_pad, u64 *__restrict__ partial, unsigned *__restrict__ tau_shared,
    int ib, int item_base, int nqb, OrderArgs ord FDR_DBG_PARAM) {
#ifndef FDR_DEV
    constexpr int dbg = 0;
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int QW = 32 * NQ * NW;
    constexpr int NCH = DP / 128;            // 128-component chunks (= units) per tile
    // work item = (target segment, query block), segment-major; a launch covers the items item_base .. of a
    // one-dimensional grid (see launch_knn_prefilter: launches of at most one workgroup per resident slot)
    const int item = item_base + (int)blockIdx.x;
    const int seg = item / nqb, qb = item - seg * nqb;
    constexpr int UNIT_BYTES = 32 * 256;
    constexpr int STAGE_BYTES = U * UNIT_BYTES;  // U units per stage
    constexpr int ROW_BYTES = DP * 2;
    static_assert(NCH % U == 0 || U % NCH == 0, "a stage holds whole tiles or a tile spans whole stages");
    static_assert(NCH <= 2 * U, "a tile spans at most two stages (the loop is unrolled by stage parity)");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: LDS-DMA destinations stay in SGPRs
    const int j = lane & 31, h = lane >> 5;
    const int ql0 = wave * 32 * NQ + j;               // query set n: ql0 + 32 n
    const int qg0 = qb * QW + ql0;

    f16x8 b[NQ][NCH * 8];  // B fragments: chunk c, k-step s covers components 128c + 16s + 8h .. + 7
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const int qg = qg0 + 32 * n;
        const f16x8 *qp = reinterpret_cast<const f16x8 *>(Qh + (size_t)(qg < nq ? qg : nq - 1) * DP);
#pragma unroll
        for (int i = 0; i < NCH * 8; ++i) b[n][i] = qp[2 * i + h];
    }
    // quantisation grid and the lists (knn_prefilter_pp_kernel carries a COPY of this list code -- share, rethreshold,
    // flush, offer, the write-out: a fix here must be made there too; why it is not one struct: docs/experiments.md A-21)
    const int qbits = min(20, 32 - ib);
    const unsigned QM1 = (1u << qbits) - 2u;
    const float qscale = (float)QM1, qinv = 1.0f / qscale;
    const int nlive = (K - h + 1) >> 1, dead = LH - nlive;  // live entries of this half
    RegList<LH> L[NQ];
    unsigned flim[NQ];  // cross-segment bound on qd (admits qd <= flim); QM1 + 1 = none
    int cthr[NQ];       // a similarity can enter only if its bit pattern, as a signed int, is >= cthr
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
#pragma unroll
        for (int e = 0; e < LH; ++e) L[n].v[e] = e < dead ? 0u : PK_EMPTY;
        L[n].pmax = PK_EMPTY;
    }
    // bound exchange (see topk_share): publish the list maximum's qd once the list is full
    auto share = [&](RegList<LH> &Ln, unsigned &fl, int n) {
        unsigned *slot = tau_shared + qg0 + 32 * n;
        const unsigned tk = max(Ln.v[LH - 1], Ln.pmax);
        const unsigned mine = tk == PK_EMPTY ? 0x7F800000u : (tk >> ib);
        unsigned seen = mine;
        if (h == 0) {
            const unsigned old = mine <= QM1
                                     ? __hip_atomic_fetch_min(slot, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                     : __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            seen = min(old, mine);
        }
        const unsigned ps = partner32(seen, h);
        fl = min(h ? ps : seen, QM1 + 1);
    };
    // Threshold below which no row of a LATER tile can enter.  Rows arrive in ascending order, so a
    // later row with the list maximum's qd has a larger key than the maximum: the own bound is strict
    // (qd < maximum's qd) -- which is what keeps plateaus (e.g. an all-zero query, every similarity 0)
    // on the fast path.  The cross-segment bound admits ties.  As a similarity the threshold is
    // ((QM1 - lim) - 0.75) / QM1 > 0 (a quarter step below the rounding boundary of the last admitted
    // grid value), or -inf (everything enters), or +inf (nothing does).  Positive floats order like
    // their bit patterns and a negative similarity has a negative pattern, so the test is one signed
    // integer compare: INT_MIN = everything, INT_MAX = nothing.
    auto rethreshold = [&](const RegList<LH> &Ln, unsigned fl) -> int {
        const unsigned tk = max(Ln.v[LH - 1], Ln.pmax);
        const unsigned oq = tk >> ib;
        const unsigned lim = tk == PK_EMPTY ? fl : min(oq - 1u, fl);  // (oq == 0: wraps, handled below)
        int th = lim >= QM1 ? (int)0x80000000u : __float_as_int(((float)(QM1 - lim) - 0.75f) * qinv) + 1;
        if (tk != PK_EMPTY && oq == 0u) th = 0x7fffffff;
        return th;
    };
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        share(L[n], flim[n], n);
        cthr[n] = rethreshold(L[n], flim[n]);
        if (dbg & 16) cthr[n] = 0x7fffffff;  // (development: the real test and branch, but nothing ever passes)
    }

    const int t_begin = segs.b[seg];
    const int t_end = min(nt, segs.b[seg + 1]);
    const int ntiles = (t_end - t_begin + 31) >> 5;
    const int nunits = ntiles * NCH;
    const int nstages = (nunits + U - 1) / U;

    // LDS-DMA: piece p = wave + NW*u (1 KiB: unit p>>3 of the stage, rows 4*(p&7)..+3 of that unit,
    // 16 lanes per row; the 16-byte slot a lane fetches is XOR-swizzled with the row).  Sources are
    // 32-bit byte offsets from the segment's first row (segments are at most 2^19 rows of <= 1 KiB);
    // rows past the segment end are clamped to its last row (and masked when the tile is scored).
    constexpr int PPW = 8 * U / NW;  // pieces per wave per stage
    static_assert((8 * U) % NW == 0, "unsupported wave count");
    const char *seg_base = reinterpret_cast<const char *>(Th + (size_t)t_begin * DP);
    const unsigned last_row_off = (unsigned)(t_end - 1 - t_begin) * ROW_BYTES;
    // With eight waves piece p = wave + 8 u is unit u of the stage and a lane's row and slot inside the unit are the same for
    // every u: ONE (row, slot) pair per lane plus literals (ONEPAIR) instead of a pair per piece -- at four pieces per wave
    // the six registers spared are what keeps the 128-register shape from spilling query fragments into the loop.
    constexpr bool ONEPAIR = NW == 8 && NCH <= U;
    constexpr int NOFF = ONEPAIR ? 1 : PPW;
    unsigned soff[NOFF];  // this lane's source row (as a byte offset) for the stage issued next
    unsigned scol[NOFF];  // its byte offset inside the row
#pragma unroll
    for (int u = 0; u < NOFF; ++u) {
        const int piece = wave + NW * u;
        const int row = 4 * (piece & 7) + (lane >> 4), pslot = lane & 15;
        // unit piece>>3 of a stage: tile (piece>>3) / NCH of the stage (NCH <= U), chunk (piece>>3) % NCH
        // (+ U per odd stage when a tile spans two stages)
        scol[u] = (unsigned)((pslot ^ (row & 15)) * 16 + ((piece >> 3) % NCH) * 256);
        soff[u] = (unsigned)(32 * ((piece >> 3) / NCH) + row) * ROW_BYTES;
    }
    auto issue_stage = [&](auto par_c) {  // par = parity of the stage being issued
        constexpr int par = decltype(par_c)::value;
        unsigned char *dst = smem + par * STAGE_BYTES;
        if constexpr (ONEPAIR) {
            static_for(std::make_integer_sequence<int, PPW>{}, [&](auto u_c) {
                constexpr int u = decltype(u_c)::value;  // (= the unit: piece = wave + 8 u)
                constexpr unsigned row_c = (unsigned)(32 * (u / NCH)) * ROW_BYTES, col_c = (unsigned)((u % NCH) * 256);
                unsigned vrow = soff[0];
                asm volatile("" : "+v"(vrow));  // (opaque: otherwise hipcc keeps soff + row_c of every piece in a register of its own)
                const unsigned off = min(vrow + row_c, last_row_off) + scol[0] + col_c;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(seg_base + off),
                                                 (__attribute__((address_space(3))) void *)(dst + (wave + NW * u) * 1024),
                                                 16, 0, 0);
            });
            soff[0] += (unsigned)(32 * (U / NCH)) * ROW_BYTES;  // U / NCH tiles further
        } else {
#pragma unroll
            for (int u = 0; u < PPW; ++u) {
                const int piece = wave + NW * u;
                const unsigned off = min(soff[u], last_row_off) + scol[u] + (NCH > U ? par * U * 256 : 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(seg_base + off),
                                                 (__attribute__((address_space(3))) void *)(dst + piece * 1024),
                                                 16, 0, 0);
                if constexpr (NCH <= U) soff[u] += (unsigned)(32 * (U / NCH)) * ROW_BYTES;  // U / NCH tiles further
                else if constexpr (par == 1) soff[u] += (unsigned)32 * ROW_BYTES;  // second half done: next tile
            }
        }
    };
    if (nstages > 0) issue_stage(std::integral_constant<int, 0>{});
    __syncthreads();  // (hipcc drains the DMA before the barrier)

    // Candidates wait in a two-entry queue per lane (registers) and enter the lists in batches: late in a
    // scan a tile offers ~1 candidate to ONE of the wave's 32 queries, and a round costs the same for 1
    // query as for 32.  A flush drains the queues with at most four rounds.  Queued candidates are not
    // reflected in the threshold: it is only looser for that, never wrong.
    unsigned q0[NQ], q1[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) q0[n] = q1[n] = PK_EMPTY;
    auto flush = [&](RegList<LH> &Ln, unsigned &a0, unsigned &a1) {
        const bool dbgc = (dbg & 2) != 0;
        while (__any(a0 != PK_EMPTY)) {
            DBG_COUNT(4);
            const unsigned took = reglist_round<LH>(Ln, a0, h);  // the smaller head of the query's two lanes
            if (a0 == took) {
                a0 = a1;
                a1 = PK_EMPTY;
            }
        }
    };
    // the rows of one finished tile against query set n's list (cold: most tiles have no candidate)
    auto offer = [&](const f32x16 &a, const int (&g)[4], RegList<LH> &Ln, unsigned &a0, unsigned &a1,
                     const unsigned fl, const int th, int lrow, int nvalid) {
        const bool dbgc = (dbg & 2) != 0;
        DBG_COUNT(1);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            if (!__any(g[q4] >= th)) continue;
            DBG_COUNT(2);
#pragma unroll
            for (int r = 4 * q4; r < 4 * q4 + 4; ++r) {
                const int roff = (r & 3) + 8 * (r >> 2);
                const bool pass = __float_as_int(a[r]) >= th && roff + 4 * h < nvalid;
                if (!__any(pass)) continue;
                unsigned cand = PK_EMPTY;
                if (pass) {
                    const float sc = fminf(fmaxf(a[r], 0.0f), 1.0f);
                    const unsigned qd = QM1 - (unsigned)__builtin_rintf(sc * qscale);
                    if (qd <= fl) cand = (qd << ib) | (unsigned)(lrow + roff);
                }
                DBG_COUNT(3);
                if (__any(cand != PK_EMPTY && a1 != PK_EMPTY)) flush(Ln, a0, a1);  // some lane's queue is full
                a1 = (a0 != PK_EMPTY && a1 == PK_EMPTY) ? cand : a1;
                a0 = a0 == PK_EMPTY ? cand : a0;
            }
        }
    };
    typedef const f16x8 __attribute__((address_space(3))) lds_f16x8;
    unsigned fa[8];
    fragment_addresses(fa, smem, j, h);

    f32x16 acc[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

    // score one finished tile of query set n (hot: a max tree and one compare; cold: offer())
    auto score = [&](const f32x16 &av, int n, int t) __attribute__((always_inline)) {
        int g[4];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
            g[q4] = max(max(max(__float_as_int(av[4 * q4]), __float_as_int(av[4 * q4 + 1])),
                            __float_as_int(av[4 * q4 + 2])),
                        __float_as_int(av[4 * q4 + 3]));
        const int mx = max(max(max(g[0], g[1]), g[2]), g[3]);
        const bool dbgc = (dbg & 2) != 0;
        DBG_COUNT(0);
        if (dbg & 1) {  // timing experiment: MFMA + fast path only
            if (mx == 0x7fffffff) cthr[n] = mx;
        } else if (__any(mx >= cthr[n])) {
            int lrow = t * 32 + 4 * h;  // row - segment start of this lane's first row
            int nvalid = t_end - (t_begin + t * 32);
            asm volatile("" : "+v"(lrow), "+s"(nvalid));  // keep the cold block's set-up cold
            offer(av, g, L[n], q0[n], q1[n], flim[n], cthr[n], lrow, nvalid);
            cthr[n] = rethreshold(L[n], flim[n]);
        }
    };
    constexpr bool PAIR = PAIRED && NCH == 1 && (U == 2 || U == 4) && NQ == 1;  // a stage's tiles pairwise as two MFMA chains
    constexpr int NP = U / 2;  // ... pairs per stage (U = 4: half the barriers per tile)
    constexpr bool STAGGER = PAIR && NW == 8;  // the eight-wave shape's second half scores a stage late (below)
    const bool late = STAGGER && wave >= NW / 2;  // (wave-uniform)
    f32x16 accB;  // PAIR: the second tile's accumulators
#pragma unroll
    for (int r = 0; r < 16; ++r) accB[r] = 0.f;
#ifdef FDR_STAMPS
    unsigned stamp_acc[6] = {0, 0, 0, 0, 0, 0};
    const bool stamp_on = blockIdx.x == 0;
#endif
    auto stage_body = [&](auto par_c, int it) {
        constexpr int par = decltype(par_c)::value;
        STAMP(ts0);
        if (it + 1 < nstages) issue_stage(std::integral_constant<int, par ^ 1>{});  // lands before the barrier below
        STAMP(ts1);
        STAMP_ADD(0, ts0, ts1);
        if constexpr (PAIR) {
            // two independent accumulator chains (a dependent 32x32x16 MFMA waits for its predecessor's
            // result; the other tile's MFMA fills that slot); both share every query fragment
            auto mfma_pair = [&](auto p_c) __attribute__((always_inline)) {  // units 2 p, 2 p + 1 of the stage
                constexpr int OFF0 = par * STAGE_BYTES + 2 * decltype(p_c)::value * UNIT_BYTES, OFF1 = OFF0 + UNIT_BYTES;
                // software pipeline: the fragments of k-step s + 1 are requested before the MFMAs of step s
                // issue, and a step waits only for ITS two reads (counted lgkmcnt: LDS reads return in
                // order).  hipcc would wait with lgkmcnt(0), i.e. also for the reads it has just issued, so
                // the reads and the waits are written out (with four waves per SIMD the per-k-step wait
                // chain, not the matrix pipe, set the pace: 53 % of the wave cycles in s_waitcnt at 1 M rows).
                f16x8 fa0[2], fa1[2];
                lds_read128(fa0[0], fa[0], std::integral_constant<int, OFF0>{});
                lds_read128(fa1[0], fa[0], std::integral_constant<int, OFF1>{});
#pragma unroll
                for (int s8 = 0; s8 < 8; ++s8) {
                    if (s8 < 7) {
                        lds_read128(fa0[(s8 + 1) & 1], fa[s8 + 1], std::integral_constant<int, OFF0>{});
                        lds_read128(fa1[(s8 + 1) & 1], fa[s8 + 1], std::integral_constant<int, OFF1>{});
                        asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(fa0[s8 & 1]), "+v"(fa1[s8 & 1]));
                    } else {
                        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa0[s8 & 1]), "+v"(fa1[s8 & 1]));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    // (the first k-step accumulates onto an inline 0: no 2 x 16 v_mov per stage to clear the accumulators)
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0[s8 & 1], b[0][s8], s8 == 0 ? f32x16{} : acc[0], 0, 0, 0);
                    accB = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1[s8 & 1], b[0][s8], s8 == 0 ? f32x16{} : accB, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            auto score_pair = [&](const int ts) __attribute__((always_inline)) {
                score(acc[0], 0, ts);
                if (ts + 1 < nunits) score(accB, 0, ts + 1);  // (the second unit of a last, odd pair is padding)
            };
            if constexpr (STAGGER) {
                // Staggered halves (eight waves: two per SIMD run the same program with one barrier per stage and would
                // reach their MFMAs, their LDS reads and their scoring together): waves 4 .. 7 score a pair of tiles one
                // pair LATER -- a stage's last pair at the start of the next stage, the accumulators simply stay in their
                // registers across the barrier -- so that on every SIMD one wave of the pair is in its vector part while
                // the other feeds the matrix pipe.  One more (MFMA-less) iteration lets them score the last stage's.
                if (late && it > 0 && U * it - 2 < nunits) score_pair(U * it - 2);
                if (it < nstages) {
                    static_for(std::make_integer_sequence<int, NP>{}, [&](auto p_c) {
                        constexpr int p = decltype(p_c)::value;
                        const int tp = U * it + 2 * p;
                        if (tp < nunits) {  // (wave-uniform; a segment's last stage may hold one pair only)
                            mfma_pair(p_c);
                            if (!late || p < NP - 1) score_pair(tp);
                        }
                    });
                }
            } else {
                static_for(std::make_integer_sequence<int, NP>{}, [&](auto p_c) {
                    const int tp = U * it + 2 * decltype(p_c)::value;
                    if (tp < nunits) {
                        mfma_pair(p_c);
                        score_pair(tp);
                    }
                });
            }
        } else {
        // (also the 168-VGPR d <= 256 shape with 16-key lists, two k-steps deep: 322 -> 315 ms at 1 M doubled rows, k = 20;
        // d <= 128 with 32-key lists at 128 VGPRs spills: 42 -> 204 ms)
        constexpr bool DEEP = WPS <= 2 || (WPS == 3 && DP == 256 && LH == 16);
        if (DEEP && U * (it + 1) <= nunits) {  // (a full stage; a segment's last, partial one: below)
            // 256-register shapes (two waves per SIMD: little else hides an LDS latency): ONE continuous pipeline over the
            // stage's 8 U k-steps -- the fragment of k-step s + D is requested before the MFMA of k-step s issues, and a
            // k-step waits only for ITS read (counted lgkmcnt: LDS reads return in order), across unit and tile
            // boundaries.  D + 1 fragment registers instead of eight, no bubble per unit.
            if constexpr (DEEP) {
                constexpr int KS = 8 * U, D = WPS <= 2 ? 4 : 2, R = D + 1;  // D: k-steps the fragments are read ahead
                f16x8 fr[R];
                // (a ring beyond 64 KB: the odd stage's base no longer fits the 16-bit immediate; its addresses are made once
                // per stage)
                constexpr bool FAR = STAGE_BYTES * 2 > 65536;
                unsigned fb[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) fb[i] = FAR ? fa[i] + (unsigned)(par * STAGE_BYTES) : fa[i];
                auto rd = [&](auto s_c) __attribute__((always_inline)) {
                    constexpr int s = decltype(s_c)::value;
                    lds_read128(fr[s % R], fb[s % 8],
                                std::integral_constant<int, (FAR ? 0 : par * STAGE_BYTES) + (s / 8) * UNIT_BYTES>{});
                };
                static_for(std::make_integer_sequence<int, D>{}, rd);
                auto kstep = [&](auto s_c) __attribute__((always_inline)) {
                    constexpr int s = decltype(s_c)::value;
                    constexpr int uu = s / 8, s8 = s % 8;
                    constexpr int c = NCH <= U ? uu % NCH : (U * par + uu) % NCH;  // static chunk number
                    if constexpr (s + D < KS) rd(std::integral_constant<int, s + D>{});
                    wait_lgkmcnt<(KS - 1 - s < D ? KS - 1 - s : D)>(fr[s % R]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int n = 0; n < NQ; ++n)  // (a tile's first k-step accumulates onto an inline 0)
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[s % R], b[n][c * 8 + s8],
                                                                        (c == 0 && s8 == 0) ? f32x16{} : acc[n], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (s8 == 7 && c == NCH - 1) {
                        const int t = (U * it + uu) / NCH;
#pragma unroll
                        for (int n = 0; n < NQ; ++n) score(acc[n], n, t);
                    }
                };
                static_for(std::make_integer_sequence<int, KS>{}, kstep);
            }
        } else {
#pragma unroll
        for (int uu = 0; uu < U; ++uu) {
            const int c = NCH <= U ? uu % NCH : (U * par + uu) % NCH;  // static chunk number
            const int unit = U * it + uu;
            if (unit < nunits) {  // wave-uniform
                const int t = unit / NCH;
                if (c == 0) {
#pragma unroll
                    for (int n = 0; n < NQ; ++n)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
                }
                if constexpr (WPS <= 2) {  // 256 registers: all eight fragments in flight (+5 % at d = 500; at three or
                                           // four waves per SIMD: no gain at d = 256 / K' <= 32, spills at d = 128 / K' > 32)
                    f16x8 a[8];
#pragma unroll
                    for (int s8 = 0; s8 < 8; ++s8)
                        a[s8] = *(lds_f16x8 *)(size_t)(fa[s8] + (unsigned)(par * STAGE_BYTES + uu * UNIT_BYTES));
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int s8 = 0; s8 < 8; ++s8)
#pragma unroll
                        for (int n = 0; n < NQ; ++n)
                            acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s8], b[n][c * 8 + s8], acc[n], 0, 0, 0);
                } else {
#pragma unroll
                    for (int s8 = 0; s8 < 8; ++s8) {
                        const f16x8 a = *(lds_f16x8 *)(size_t)(fa[s8] + (unsigned)(par * STAGE_BYTES + uu * UNIT_BYTES));
#pragma unroll
                        for (int n = 0; n < NQ; ++n)
                            acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b[n][c * 8 + s8], acc[n], 0, 0, 0);
                    }
                }
                if (c == NCH - 1) {
                    // acc[n][r] = similarity of query j of set n with tile row (r&3) + 8*(r>>2) + 4*h
#pragma unroll
                    for (int n = 0; n < NQ; ++n) score(acc[n], n, t);
                }
            }
        }
        }
        }
        STAMP(ts2);
        STAMP_ADD(1, ts1, ts2);
        if ((it & FDR_SHARE_EVERY) == FDR_SHARE_EVERY) {
#pragma unroll
            for (int n = 0; n < NQ; ++n) {
                flush(L[n], q0[n], q1[n]);
                share(L[n], flim[n], n);
                cthr[n] = rethreshold(L[n], flim[n]);
                if (dbg & 16) cthr[n] = 0x7fffffff;
            }
        }
        STAMP(ts3);
        STAMP_ADD(2, ts2, ts3);
#ifdef FDR_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the DMA's landing apart from the barrier's skew)
        STAMP(ts3b);
        STAMP_ADD(3, ts3, ts3b);
        __syncthreads();
        STAMP(ts4);
        STAMP_ADD(4, ts3b, ts4);
        if (stamp_on) stamp_acc[5] += 1;
#else
        __syncthreads();  // stage it+1 is complete (all waves' pieces) before anyone reads it
#endif
    };
    const int niter = nstages + (STAGGER ? 1 : 0);
    for (int it0 = 0; it0 < niter; it0 += 2) {
        stage_body(std::integral_constant<int, 0>{}, it0);
        if (it0 + 1 < niter) stage_body(std::integral_constant<int, 1>{}, it0 + 1);
    }
#ifdef FDR_STAMPS
    if (stamp_on && lane == 0)
        for (int ph = 0; ph < 6; ++ph) atomicAdd(&g_stamps[wave][ph], (unsigned long long)stamp_acc[ph]);
#endif
    const unsigned imask = (1u << ib) - 1u;
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        flush(L[n], q0[n], q1[n]);
        size_t qrow = (size_t)qb * QW + ql0 + 32 * n;
        if (ord.perm_q) {  // (ordered scan: the lists are written at the query's own row, with the targets' own rows)
            if (qrow >= (size_t)nq) continue;
            qrow = (size_t)ord.perm_q[qrow];
        }
        u64 *out = partial + ((size_t)seg * nq_pad + qrow) * K + (h ? (K + 1) >> 1 : 0);
#pragma unroll
        for (int e = 0; e < LH; ++e) {
            if (e >= dead) {
                const unsigned kv = L[n].v[e];
                u64 o = KEY_INF;
                if (kv != PK_EMPTY) {
                    int trow = t_begin + (int)(kv & imask);
                    if (ord.perm_t) trow = ord.perm_t[trow];
                    o = ((u64)__float_as_uint((float)(kv >> ib) / qscale) << 32) | (unsigned)(t_base + trow);
                }
                out[e - dead] = o;
            }
        }
    }
}

// The value lane ^ J holds, on the vector ALU (DPP row operations, v_permlane16/32_swap) instead of ds_bpermute:
// the sorts below are 21 / 28 exchange stages of 64-bit keys per call and run once or twice per query in the
// merge, re-rank and expansion kernels, where the LDS pipe (one per CU, shared by four SIMDs) was their bound.
template <int J>
__device__ __forceinline__ unsigned lane_xor(unsigned v, const int lane) {
    static_assert(J == 1 || J == 2 || J == 4 || J == 8 || J == 16 || J == 32, "a power of two below 64");
    if constexpr (J == 1) {
        return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);  // quad_perm:[1,0,3,2]
    } else if constexpr (J == 2) {
        return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);  // quad_perm:[2,3,0,1]
    } else if constexpr (J == 4) {
        const int up = __builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xF, 0xF, true);  // row_shl:4 (lane i reads lane i + 4)
        const int dn = __builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);  // row_shr:4 (lane i reads lane i - 4)
        return (unsigned)((lane & 4) ? dn : up);
    } else if constexpr (J == 8) {
        return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, true);  // row_ror:8
    } else if constexpr (J == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // rows 0 <-> 1 and 2 <-> 3
        return (lane & 16) ? r[0] : r[1];
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (lane & 32) ? r[0] : r[1];
    }
}
template <int J>
__device__ __forceinline__ u64 lane_xor64(u64 v, const int lane) {
    return ((u64)lane_xor<J>((unsigned)(v >> 32), lane) << 32) | lane_xor<J>((unsigned)v, lane);
}

// The stages k = KMIN .. KMAX of the bitonic sorting network over the lanes (u64 keys, one per lane); blocks of
// KMAX lanes end up ascending.  <2, 64>: a full sort (21 compare-exchange stages); <2, 32>: each half-wave sorted
// by itself (15 stages); <32, 64>: the input already consists of runs of 16 lanes, ascending in the even runs and
// descending in the odd ones -- what the stages below 32 would have produced (11 stages).
template <int KMIN, int KMAX>
__device__ __forceinline__ u64 wave_bitonic(u64 key, const int lane) {
    static_for(std::integer_sequence<int, 2, 4, 8, 16, 32, 64>{}, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if constexpr (k >= KMIN && k <= KMAX) {
            static_for(std::make_integer_sequence<int, 6>{}, [&](auto sc) {
                constexpr int j = (k >> 1) >> decltype(sc)::value;
                if constexpr (j > 0) {
                    const u64 other = lane_xor64<j>(key, lane);
                    const bool up = k == KMAX || (lane & k) == 0;
                    const bool take_min = ((lane & j) == 0) == up;
                    key = (take_min == (other < key)) ? other : key;
                }
            });
        }
    });
    return key;
}
// Ascending sort of one u64 key per lane across the wave.
__device__ __forceinline__ u64 wave_sort64(u64 key, const int lane) { return wave_bitonic<2, 64>(key, lane); }
// ... across each half-wave by itself (keys of interest in lanes 0 .. 31, the other half unused or another set).
__device__ __forceinline__ u64 wave_sort32(u64 key, const int lane) { return wave_bitonic<2, 32>(key, lane); }

// Ascending bitonic sort of 128 keys, two per lane: a = element `lane`, b = element `lane + 64`.
__device__ __forceinline__ void wave_sort128(u64 &a, u64 &b, const int lane) {
    static_for(std::integer_sequence<int, 2, 4, 8, 16, 32, 64, 128>{}, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        static_for(std::make_integer_sequence<int, 7>{}, [&](auto sc) {
            constexpr int j = (k >> 1) >> decltype(sc)::value;
            if constexpr (j == 64) {  // (k == 128: ascending) partner = the lane's other element
                const u64 lo = a < b ? a : b, hi = a < b ? b : a;
                a = lo;
                b = hi;
            } else if constexpr (j > 0) {
                const u64 oa = lane_xor64<j>(a, lane), ob = lane_xor64<j>(b, lane);
                const bool up_a = k >= 64 || (lane & k) == 0;               // direction of element lane
                const bool up_b = k == 128 || (k < 64 && (lane & k) == 0);  // ... of element lane + 64
                const bool lower = (lane & j) == 0;
                a = ((lower == up_a) == (oa < a)) ? oa : a;
                b = ((lower == up_b) == (ob < b)) ? ob : b;
            }
        });
    });
}

// P1's merge: the KP smallest keys of a query's nseg segment lists, sorted.  One wave per query.
// A segment list arrives as two ascending halves ([0, ceil(KP/2)) and the rest; KEY_INF = empty slot),
// so a full list's maximum is the larger of the two last entries, and the smallest such maximum over
// the segments bounds the query's KP-th key.  About KP * (rows / rows of the longest segment) keys
// survive that bound (74 of 140 for the five segments of 1 M rows; the bound is taken over ALL segments, up to 96); they are compacted into LDS, the first 64
// are sorted with a 64-lane bitonic network, whose KP-th key is a tighter bound for the rest, and a
// second sort of the KP best + the few remaining survivors finishes.  More than 128 survivors (wide
// plateaus), more than 64 in the second sort, or no full list: KP rounds of a wave-wide minimum.
// The queries a launch of the merge or the re-rank works on: all nq of the call (perm == null: item i is query i, n =
// nq), or the `n` = 256 x blocks items of a list of 256-query blocks of the scan order -- item i is position
// blocks[i / 256] * 256 + i % 256 (blocks == null: position i, the gathered dense group) and query perm[position];
// positions from `limit` on hold no query (the short last block).  The live-chunk pass's groups are such lists
// (PrefilterCall::group_queries), so that a finished group's queries are merged and re-ranked while later groups run.
struct QuerySel {
    const int *blocks, *perm;
    int n, limit;
};
__device__ __forceinline__ int sel_query(const QuerySel &s, int i) {  // item i's query, -1: none
    if (i >= s.n) return -1;
    if (!s.perm) return i;
    const int pos = s.blocks ? s.blocks[i >> 8] * 256 + (i & 255) : i;
    return pos < s.limit ? s.perm[pos] : -1;
}
#define MERGE_QPW 4  // queries per wave when every key of a query has a lane (nseg * KP <= 64)
#define MERGE_ADAPTIVE_FROM 8  // more lists per query than this: the adaptive bound (see knn_merge_keys_kernel)
// the value lane 63 - l holds (a run reversed), for the bitonic merge of two ascending runs
__device__ __forceinline__ u64 lane_reverse64(u64 v, const int lane) {
    u64 r = v;
    r = lane_xor64<1>(r, lane);
    r = lane_xor64<2>(r, lane);
    r = lane_xor64<4>(r, lane);
    r = lane_xor64<8>(r, lane);
    r = lane_xor64<16>(r, lane);
    r = lane_xor64<32>(r, lane);
    return r;
}
__global__ __launch_bounds__(256) void knn_merge_keys_kernel(const u64 *__restrict__ partial, int nseg,
                                                             QuerySel sel, int nq_pad, int KP,
                                                             u64 *__restrict__ cand) {
    __shared__ u64 stage[4][MERGE_CAP];
    static_assert(MERGE_CAP >= 256, "a wave's stage row doubles as its survivor buffer (256 keys)");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int M = nseg * KP;
    if (M <= 64) {
        // One or two segments of short lists (1 M rows, k = 20): every key has a lane, one sort, no bound; the work
        // of a query is so small that a wave takes MERGE_QPW of them, their loads and sorts interleaved (the grid
        // is sized accordingly: merge_keys_blocks).
        const int q0 = (blockIdx.x * 4 + wave) * MERGE_QPW;
        // K' = 32: a list is two ascending runs of 16 keys (empty slots = KEY_INF last); a lane of an odd run takes
        // its run's elements from the back, and what is left of the sort is the merge of four runs (11 stages of 21).
        // (An ordered scan leaves a run sorted by distance and SCAN position: as (distance, row) keys its ties are in
        // any order.  For every distance threshold the runs are still bitonic 0-1 sequences, so the network's output
        // is sorted by distance with ties in some fixed order -- all the re-rank reads from it: d~(K), d~(K'), and
        // the set of candidates below a distance bound, which excludes the K'-th distance itself.)
        const bool runs16 = KP == 32;
        const int sg = lane / KP;
        const int e = runs16 && (lane & 16) ? (lane & 16) + 15 - (lane & 15) : lane - sg * KP;
        u64 kv[MERGE_QPW];
        int qs[MERGE_QPW];
#pragma unroll
        for (int t = 0; t < MERGE_QPW; ++t) qs[t] = sel_query(sel, q0 + t);
#pragma unroll
        for (int t = 0; t < MERGE_QPW; ++t)
            kv[t] = (lane < M && qs[t] >= 0) ? partial[((size_t)sg * nq_pad + qs[t]) * KP + e] : KEY_INF;
        if (runs16) {
#pragma unroll
            for (int t = 0; t < MERGE_QPW; ++t) kv[t] = wave_bitonic<32, 64>(kv[t], lane);
        } else {
#pragma unroll
            for (int t = 0; t < MERGE_QPW; ++t) kv[t] = wave_sort64(kv[t], lane);
        }
#pragma unroll
        for (int t = 0; t < MERGE_QPW; ++t)
            if (lane < KP && qs[t] >= 0) cand[(size_t)qs[t] * KP + lane] = kv[t];
        return;
    }
    u64 *sv = stage[wave];
    const int q = sel_query(sel, blockIdx.x * 4 + wave);
    if (q < 0) return;
    if (nseg > MERGE_ADAPTIVE_FROM) {
        // Many segments (a rank of config 5: 39-48 lists of 62 keys per query): the static bound below -- the smallest
        // maximum of a FULL list -- sits near the (nseg * KP)-th best key, a thousand keys survive it and every query
        // fell through to KP rounds of wave-wide minima over all nseg * KP keys (263 ms of a 9.2 s rank step).  Instead
        // the bound ADAPTS: `best` holds the 64 smallest keys met so far, ascending, one per lane; a list's keys are kept
        // only if they beat its KP-th, kept keys gather in LDS, and every 64 of them are sorted and merged into `best`
        // (the elementwise minimum of an ascending and a descending run is bitonic: six more stages sort it).  After the
        // first two lists almost nothing survives; a query costs its loads and a few sorts.
        u64 best = KEY_INF, bound = KEY_INF;
        int pc = 0;  // keys waiting in sv (wave-uniform)
        auto merge64 = [&]() {  // sv[0 .. 64) (KEY_INF-padded) into best; the rest of sv moves to the front
            const u64 srt = wave_sort64(sv[lane], lane);
            const u64 rev = lane_reverse64(srt, lane);
            best = wave_bitonic<64, 64>(rev < best ? rev : best, lane);
            bound = __shfl(best, KP - 1);
            const u64 tail = sv[64 + lane];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            sv[lane] = tail;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        u64 kvs[8];
        for (int sg0 = 0; sg0 < nseg; sg0 += 8) {
#pragma unroll
            for (int i = 0; i < 8; ++i)  // (eight lists' keys in flight together)
                kvs[i] = (lane < KP && sg0 + i < nseg) ? partial[((size_t)(sg0 + i) * nq_pad + q) * KP + lane] : KEY_INF;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const u64 kv = kvs[i];
                const bool keep = kv < KEY_INF && kv <= bound;
                const u64 mask = __ballot(keep);
                if (mask == 0ull) continue;  // (wave-uniform)
                if (keep) sv[pc + __popcll(mask & ((1ull << lane) - 1ull))] = kv;
                pc += __popcll(mask);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (pc >= 64) {  // (pc <= 63 + KP <= 127: one merge empties the first 64)
                    if (pc < 128 && lane >= pc - 64) sv[64 + lane] = KEY_INF;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    merge64();
                    pc -= 64;
                }
            }
        }
        if (pc > 0) {
            if (lane >= pc) sv[lane] = KEY_INF;
            sv[64 + lane] = KEY_INF;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            merge64();
        }
        if (lane < KP) cand[(size_t)q * KP + lane] = best;
        return;
    }
    {
        // (the first eight segments' keys and the bound's operands are all in flight together)
        u64 kvs[8];
        auto load_batch = [&](int sg0) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                kvs[i] = (lane < KP && sg0 + i < nseg) ? partial[((size_t)(sg0 + i) * nq_pad + q) * KP + lane]
                                                       : KEY_INF;
        };
        load_batch(0);
        u64 bound = KEY_INF;
        for (int sg = lane; sg < nseg; sg += 64) {  // (up to FDR_MAX_SEG = 96 segments: a lane may own two)
            const u64 *l = partial + ((size_t)sg * nq_pad + q) * KP;
            const u64 a = l[((KP + 1) >> 1) - 1], b2 = l[KP - 1];
            // (every row at the maximum's distance: an ordered scan sorts a list by distance and SCAN position, so
            // among equal distances the last entry need not carry the largest row number)
            if (a != KEY_INF && b2 != KEY_INF) {
                const u64 m = (a > b2 ? a : b2) | 0xffffffffull;
                bound = m < bound ? m : bound;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(bound, off);
            bound = o < bound ? o : bound;
        }
        int total = 0;
        if (bound != KEY_INF) {
            for (int sg0 = 0;;) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const u64 kv = kvs[i];
                    const bool keep = kv <= bound;  // (bound < KEY_INF)
                    const u64 mask = __ballot(keep);
                    const int pos = total + __popcll(mask & ((1ull << lane) - 1ull));
                    if (keep && pos < 256) sv[pos] = kv;
                    total += __popcll(mask);
                }
                sg0 += 8;
                if (sg0 >= nseg) break;
                load_batch(sg0);
            }
        }
        if (bound != KEY_INF && total <= 256) {  // (total >= KP: the bounding list alone has KP such keys)
            if (total <= 64) {
                const u64 kv = wave_sort64(lane < total ? sv[lane] : KEY_INF, lane);
                if (lane < KP) cand[(size_t)q * KP + lane] = kv;
                return;
            }
            u64 ka = sv[lane];  // (total > 64)
            u64 kb = 64 + lane < total ? sv[64 + lane] : KEY_INF;
            wave_sort128(ka, kb, lane);
            bool done = total <= 128;
            if (!done) {
                // the KP-th of the first 128 bounds what is still needed from the other (at most 128) survivors
                const u64 b2 = __shfl(ka, KP - 1);
                const u64 e0 = 128 + lane < total ? sv[128 + lane] : KEY_INF;
                const u64 e1 = 192 + lane < total ? sv[192 + lane] : KEY_INF;
                const bool k0 = e0 <= b2, k1 = e1 <= b2;
                const u64 m0 = __ballot(k0), m1 = __ballot(k1);
                const int n0 = __popcll(m0), nx = n0 + __popcll(m1);
                if (KP + nx <= 128) {
                    const u64 below = (1ull << lane) - 1ull;
                    if (lane < KP) sv[lane] = ka;
                    if (k0) sv[KP + __popcll(m0 & below)] = e0;
                    if (k1) sv[KP + n0 + __popcll(m1 & below)] = e1;
                    ka = lane < KP + nx ? sv[lane] : KEY_INF;
                    kb = 64 + lane < KP + nx ? sv[64 + lane] : KEY_INF;
                    wave_sort128(ka, kb, lane);
                    done = true;
                }
            }
            if (done) {
                if (lane < KP) cand[(size_t)q * KP + lane] = ka;  // (KP <= 64: the first element of each lane)
                return;
            }
        }
    }
    const bool staged = M <= MERGE_CAP;
    u64 *mine_lds = stage[wave];
    auto key_at = [&](int m) -> u64 {
        const int seg = m / KP, e = m - seg * KP;
        return partial[((size_t)seg * nq_pad + q) * KP + e];
    };
    if (staged)
        for (int m = lane; m < M; m += 64) mine_lds[m] = key_at(m);
    u64 prev1 = 0, mine = KEY_INF;
    for (int r = 0; r < KP; ++r) {
        u64 best = ~0ull;
        for (int m = lane; m < M; m += 64) {
            u64 kv;
            kv = staged ? mine_lds[m] : key_at(m);
            if (kv + 1 > prev1 && kv < best) best = kv;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(best, off);
            best = o < best ? o : best;
        }
        // several KEY_INF entries (lists that never filled) are not unique: stop advancing there
        if (best >= KEY_INF) best = KEY_INF; else prev1 = best + 1;
        if (lane == r) mine = best;
    }
    if (lane < KP) cand[(size_t)q * KP + lane] = mine;
}

// P2: certificate + exact re-rank.  One wave per query, one lane per candidate.
// The candidates' fp32 rows are fetched by the whole wave, 128 components of ROWS rows at a time (a half-wave per
// row and load: whole 512-byte runs instead of 16 bytes from each of K' rows), and turned through LDS (rows
// RERANK_STRIDE floats apart: lane r reading row r meets no bank conflict) so that each lane still runs the
// canonical chain of its own candidate; the query row is wave-uniform and read through the scalar cache.
//
// Compact route (rc != null; DP = RC_DP): a needed candidate's lane reads the row's own record instead (knn_workspace.inc:
// RC_*, written by to_half_compact_kernel) and runs c = fmaf(q[pos_e], val_e, c) over its entries in record order --
// the dense chain with the terms of the zero components left out, which changes no bit (DESIGN.md section 6).  The
// query row sits in LDS for that, read with a per-lane position; the loop runs to the wave's largest count with the
// lanes past their own count predicated off, and the second half of a record is read only by the lanes whose count
// says so.  A candidate whose record is long keeps the dense route, which then fetches the long rows only.
// ROWS = rows of a dense batch (lane l's candidate is row l % ROWS of batch l / ROWS): 32 where every candidate takes the
// dense route (67.6 KB of rows a workgroup, 8 waves per CU), 16 beside the compact route, where a batch serves the few
// long rows (35.8 KB, 16 waves per CU: the record reads are latency-bound).
#define RERANK_ROWS_DENSE 32
#define RERANK_ROWS_COMPACT 16
#define RERANK_STRIDE 132
// a wave's rows and, in the instance that reads records, its query row
#define RERANK_WAVE_FLOATS(ROWS) ((ROWS) * RERANK_STRIDE + ((ROWS) == RERANK_ROWS_COMPACT ? RC_DP : 0))
#define RERANK_LDS_BYTES(ROWS) (4 * RERANK_WAVE_FLOATS(ROWS) * 4)  // four waves per workgroup
template <int ROWS>
__global__ __launch_bounds__(256) void knn_rerank_kernel(
    const u64 *__restrict__ cand, int KP, int K, const float *__restrict__ Qhat,
    const unsigned char *__restrict__ qzero, const float *__restrict__ That, int nq, int DP, int t_base,
    float margin, int *__restrict__ idx_out, float *__restrict__ dist_out, int *__restrict__ counter,
    int *__restrict__ flagged, int *__restrict__ range_list, float *__restrict__ theta,
    unsigned char *__restrict__ path,  // path[q]: how query q's result is produced (FDR_PATH_*: fdr_last_query_paths)
    const unsigned char *__restrict__ rc,  // the targets' compact records, from row t_base on (null: dense route only)
    int long_limit,  // ... read only if their build counted at most so many long rows (counter[8]; knn_workspace.inc)
    QuerySel sel) {  // the launch's queries, a wave each (several launches append to flagged / range_list alike)
    extern __shared__ float rerank_rows[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *rows = rerank_rows + wave * RERANK_WAVE_FLOATS(ROWS);
    const int q = __builtin_amdgcn_readfirstlane(sel_query(sel, blockIdx.x * 4 + wave));  // (wave-uniform)
    if (q < 0) return;
    if (qzero[q]) {  // all-zero query: closed-form answer (zero_answer_kernel); listed from the back
        if (lane == 0) {
            flagged[nq - 1 - atomicAdd(counter + 1, 1)] = q;
            path[q] = FDR_PATH_ZERO;
        }
        return;
    }
    u64 key = KEY_INF;
    if (lane < KP) key = cand[(size_t)q * KP + lane];
    const float dt = __uint_as_float((unsigned)(key >> 32));
    const float dK = __shfl(dt, K - 1), dKP = __shfl(dt, KP - 1);
    const bool valid = (dK + margin < 1.0f) && (dK + margin < dKP);
    if (!valid) {
        if (lane == 0) {
            if (range_list && dK + margin < 1.0f) {  // plateau: collect {d~ <= d~(K) + M} in a range pass
                range_list[atomicAdd(counter + 2, 1)] = q;
                theta[q] = dK + margin;
                path[q] = FDR_PATH_RANGE;
            } else {
                flagged[atomicAdd(counter, 1)] = q;
                path[q] = FDR_PATH_EXACT;
            }
        }
        return;
    }
    // A candidate with d~ > d~(K) + M has an exact distance above d~(K) + eps + 4e-7, i.e. above the exact
    // distances of the K candidates with the smallest d~: it cannot be in the top K, so its row is not read.
    if (lane == 0) path[q] = FDR_PATH_CERTIFIED;
    const bool need = lane < KP && key < KEY_INF && dt <= dK + margin;
    const int tidx = (int)(unsigned)(key & 0xffffffffull);
    u64 densemask = __ballot(need);  // the candidates of the dense route
    const int half = lane >> 5, l5 = lane & 31;
    float c = 0.0f;
    if (ROWS == RERANK_ROWS_COMPACT && rc && counter[8] <= long_limit) {  // (wave-uniform; the other instance has no query row)
        float *qs = rows + ROWS * RERANK_STRIDE;
        reinterpret_cast<float2 *>(qs)[lane] = reinterpret_cast<const float2 *>(Qhat + (size_t)q * RC_DP)[lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the wave's own LDS writes, read by its other lanes)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint4 *rec = reinterpret_cast<const uint4 *>(rc + (size_t)(need ? tidx - t_base : 0) * RC_BYTES);
        int mine = 0;  // entries this lane's chain runs over (0: not needed, or long)
        int most = 0;  // ... and the wave's largest such count (wave-uniform)
#pragma unroll
        for (int h = 0; h < RC_HALVES; ++h) {
            if (h > 0 && most <= RC_HALF_ENTRIES * h) continue;
            const bool live = h == 0 ? need : mine > RC_HALF_ENTRIES * h;
            unsigned w[16] = {};
            if (live) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint4 x = rec[4 * h + i];
                    w[4 * i] = x.x; w[4 * i + 1] = x.y; w[4 * i + 2] = x.z; w[4 * i + 3] = x.w;
                }
            }
            if (h == 0) {
                const int cnt = (int)(w[0] & 0xffu);
                mine = cnt <= RC_ENTRIES ? cnt : 0;
                densemask = __ballot(need && cnt > RC_ENTRIES);
                static_assert(RC_ENTRIES < 32, "the largest count is found over five bits");
#pragma unroll
                for (int bit = 4; bit >= 0; --bit)  // from the top bit down: does a lane that ties so far hold it?
                    if (__ballot((mine >> bit) == ((most >> bit) | 1))) most |= 1 << bit;
            }
#pragma unroll
            for (int e = 0; e < RC_HALF_ENTRIES; ++e) {
                if (RC_HALF_ENTRIES * h + e < most) {  // (wave-uniform; the lanes past their own count are predicated off)
                    const int pos = (int)((w[(1 + e) >> 2] >> (8 * ((1 + e) & 3))) & (RC_DP - 1));
                    if (RC_HALF_ENTRIES * h + e < mine) c = __builtin_fmaf(qs[pos], __uint_as_float(w[4 + e]), c);
                }
            }
        }
    }
    for (int b = 0; b * ROWS < KP; ++b) {
        const unsigned bm = (unsigned)(densemask >> (ROWS * b)) & (unsigned)((1ull << ROWS) - 1ull);
        if (!bm) continue;  // (wave-uniform)
        int trow[ROWS / 2];
#pragma unroll
        for (int it = 0; it < ROWS / 2; ++it) trow[it] = __shfl(tidx, ROWS * b + 2 * it + half) - t_base;
        for (int ch = 0; ch < DP / 128; ++ch) {
            f32x4 v[ROWS / 2];
#pragma unroll
            for (int it = 0; it < ROWS / 2; ++it) {
                v[it] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if ((bm >> (2 * it + half)) & 1u)
                    v[it] = *reinterpret_cast<const f32x4 *>(That + (size_t)trow[it] * DP + ch * 128 + l5 * 4);
            }
#pragma unroll
            for (int it = 0; it < ROWS / 2; ++it)
                *reinterpret_cast<f32x4 *>(rows + (2 * it + half) * RERANK_STRIDE + l5 * 4) = v[it];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the wave's own LDS writes, read by its other lanes)
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lane / ROWS == b && ((densemask >> lane) & 1ull)) {
                const f32x4 *tp = reinterpret_cast<const f32x4 *>(rows + (lane % ROWS) * RERANK_STRIDE);
                const f32x4 *qp = reinterpret_cast<const f32x4 *>(Qhat + (size_t)q * DP + ch * 128);
#pragma unroll
                for (int g = 0; g < 16; ++g) {  // canonical chain: components 8g .. 8g+7 of this chunk, in the kernels' order
                    const f32x4 te = tp[2 * g], to = tp[2 * g + 1];
                    const f32x4 qe = qp[2 * g], qo = qp[2 * g + 1];
                    c = __builtin_fmaf(qe.x, te.x, c);
                    c = __builtin_fmaf(qo.x, to.x, c);
                    c = __builtin_fmaf(qe.y, te.y, c);
                    c = __builtin_fmaf(qo.y, to.y, c);
                    c = __builtin_fmaf(qe.z, te.z, c);
                    c = __builtin_fmaf(qo.z, to.z, c);
                    c = __builtin_fmaf(qe.w, te.w, c);
                    c = __builtin_fmaf(qo.w, to.w, c);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (read before the next chunk overwrites the rows)
            __builtin_amdgcn_wave_barrier();
        }
    }
    u64 exact = ~0ull;
    if (need) exact = ((u64)__float_as_uint(dist_from_sim(c)) << 32) | (unsigned)tidx;
    // (distinct targets: no equal keys; unused lanes sort last; K' <= 32: the candidates sit in the first half-wave)
    const u64 mine = KP <= 32 ? wave_sort32(exact, lane) : wave_sort64(exact, lane);
    if (lane < K) {
        idx_out[(size_t)q * K + lane] = (int)(unsigned)(mine & 0xffffffffull);
        dist_out[(size_t)q * K + lane] = __uint_as_float((unsigned)(mine >> 32));
    }
}

// ---- range pass for uncertified queries --------------------------------------------------------
// A query whose K' candidates could not be certified usually sits on a plateau of (near-)ties wider
// than K' (rows with one or two non-zero components have hundreds of exact duplicates).  Its exact
// top-K is still contained in { targets with d~ <= theta }, theta = d~(K) + M (same lemma as the
// certificate, which does not need the K' list to be complete), as long as theta < 1.  This pass
// re-streams the fp16 targets for those queries only and collects that set (no top-k state at all, so
// it runs at the MFMA / staging rate); knn_rerank_long_kernel then ranks it with the canonical fp32
// chain.  Queries whose set exceeds RANGE_CAP (knn_workspace.inc) fall back to the exact kernel.
#define RANGE_STAGES 4  // LDS ring of the range pass: one-unit (8 KB) stages, RANGE_STAGES - 1 in flight
#define RANGE_LANE_BUF 8  // candidates a lane gathers in LDS before it claims their places with one atomic

// A lane's hits wait in its own RANGE_LANE_BUF-entry LDS buffer (behind the ring) and leave with ONE returning atomic per
// batch: a plateau query collects hundreds of rows, and a wave that waits ~2 us for every single `atomicAdd(cnt + q, 1)`
// spent most of a short scan doing so (1100 queries at 1 M rows / 8: 387 us).
// RangeHits is the k-NN search's sink, the default of the two range kernels; the radius search of the dense index
// runs the same kernels with a counting and an emitting one (knn_dense_radius.inc).  A sink has an Out (what the
// kernel is given for it), make(lane buffer, out, query, thread), add(row) and finish().
struct RangeOut {
    int *cnt;   // per-query hit counters
    int *cand;  // [nq][RANGE_CAP]
};
template <int NT>  // threads per workgroup = the buffer's stride
struct RangeHits {
    typedef RangeOut Out;
    int *lbuf;    // [RANGE_LANE_BUF][NT]; this lane's entries are lbuf[i * NT + tid]
    int *cnt;     // per-query hit counters
    int *cand;    // [nq][RANGE_CAP]
    int qg, tid;  // this lane's query and thread number
    int lcount;
    static __device__ __forceinline__ RangeHits make(int *lbuf, const Out &o, int qg, int tid) {
        return RangeHits{lbuf, o.cnt, o.cand, qg, tid, 0};
    }
    __device__ __forceinline__ void finish() {
        if (lcount > 0) flush();
    }
    __device__ __forceinline__ void flush() {
        const int pos = atomicAdd(cnt + qg, lcount);
        for (int i = 0; i < lcount; ++i)
            if (pos + i < RANGE_CAP) cand[(size_t)qg * RANGE_CAP + pos + i] = lbuf[i * NT + tid];
        lcount = 0;
    }
    __device__ __forceinline__ void add(int row) {
        lbuf[lcount * NT + tid] = row;
        if (++lcount == RANGE_LANE_BUF) flush();
    }
};
// the hits of one finished tile some lane of which is above its floor: acc[r] is the similarity with row
// row0 + (r & 3) + 8 * (r >> 2); sfloor is the conservative similarity form of d~ <= th
template <class Sink>
__device__ __forceinline__ void range_collect(Sink &sink, const f32x16 &acc, int row0, float sfloor, float th, int t_end,
                                              int t_base) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (acc[r] > sfloor) {
            float a1 = acc[r];
            asm volatile("" : "+v"(a1));
            const int row = row0 + (r & 3) + 8 * (r >> 2);
            if (dist_from_sim(a1) <= th && row < t_end) sink.add(t_base + row);
        }
    }
}

template <int DP, int NW, int WPS, class Sink = RangeHits<64 * NW>>
__global__ __launch_bounds__(64 * NW, WPS) void knn_range_kernel(
    const _Float16 *__restrict__ Qh, const float *__restrict__ theta, int nq,
    const _Float16 *__restrict__ Th, int nt, int t_base, SegBounds segs, const typename Sink::Out out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int QW = 32 * NW;
    constexpr int NCH = DP / 128;
    constexpr int UNIT_BYTES = 32 * 256;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int qg = blockIdx.x * QW + wave * 32 + j;
    const bool live = qg < nq;
    const int qrow = live ? qg : nq - 1;
    const float th = live ? theta[qrow] : -1.0f;          // admit d~ <= th
    const float sfloor = live ? (1.0f - th) - 3.0e-7f : __builtin_inff();  // conservative similarity form

    f16x8 b[NCH * 8];
    {
        const f16x8 *qp = reinterpret_cast<const f16x8 *>(Qh + (size_t)qrow * DP);
#pragma unroll
        for (int i = 0; i < NCH * 8; ++i) b[i] = qp[2 * i + h];
    }
    const int t_begin = segs.b[blockIdx.y];
    const int t_end = min(nt, segs.b[blockIdx.y + 1]);
    const int ntiles = (t_end - t_begin + 31) >> 5;
    const int nunits = ntiles * NCH;  // one unit per stage, two-stage ring

    // A ring of RANGE_STAGES one-unit stages, RANGE_STAGES - 1 of them in flight: the pass runs for a few query blocks
    // only (one or two workgroups per CU), so nothing but its own look-ahead hides the L2 -> LDS latency (two stages
    // and a draining barrier: 0.69 us per tile, 0.5 ms for 1100 plateau queries at 1 M rows).  A stage is awaited
    // with a counted vmcnt (LDS-DMA completes in issue order; the cold path's atomics and stores only make the wait
    // stricter) and a bare s_barrier: all waves' pieces of stage `it` are in LDS and everyone has left stage it - 1.
    constexpr int PPW = 8 / NW;
    static_assert(8 % NW == 0 && PPW * (RANGE_STAGES - 2) <= 4, "unsupported wave count");
    auto issue_stage = [&](int it) {
        unsigned char *dst = smem + (it % RANGE_STAGES) * UNIT_BYTES;
        const int t = it / NCH, c = it % NCH;
#pragma unroll
        for (int u = 0; u < PPW; ++u) {
            const int piece = wave + NW * u;
            const int row = 4 * piece + (lane >> 4), pslot = lane & 15;
            const int trow = min(t_begin + 32 * t + row, t_end - 1);
            const _Float16 *src =
                Th + (size_t)trow * DP + (size_t)(c * 128) + (size_t)((pslot ^ (row & 15)) * 8);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(dst + piece * 1024),
                                             16, 0, 0);
        }
    };
    Sink hits = Sink::make(reinterpret_cast<int *>(smem + RANGE_STAGES * UNIT_BYTES), out, qg, tid);
#pragma unroll
    for (int i = 0; i < RANGE_STAGES - 1; ++i)
        if (i < nunits) issue_stage(i);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // Fragment addresses: lane j reads slot (2 s2 + h) ^ (j & 15) of its row; the ring position is a literal offset
    // (the unit loop is unrolled over the ring), so the eight reads of a unit are ds_read_b128 with immediate offsets
    // awaited one by one with counted lgkmcnt: the first MFMA starts when the first fragment is there, not the last.
    unsigned foff[8];
    fragment_addresses(foff, smem, j, h);
    static_assert(RANGE_STAGES % NCH == 0, "the ring holds whole tiles");
    auto unit = [&](auto slotc, const int it) {
        constexpr int slot = decltype(slotc)::value;
        constexpr int c = slot % NCH;  // (RANGE_STAGES is a multiple of NCH: a unit's chunk follows from its ring slot)
        const int pending = min(RANGE_STAGES - 2, nunits - 1 - it);  // stages issued after stage `it` (wave-uniform)
        if (pending >= 2) wait_vmcnt<2 * PPW>();
        else if (pending == 1) wait_vmcnt<PPW>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (it + RANGE_STAGES - 1 < nunits) issue_stage(it + RANGE_STAGES - 1);  // (into the slot stage it - 1 has left)
        if (c == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        }
        f16x8 a[8];  // all eight fragments in flight (a read per MFMA would expose its latency eight times)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the cold path's LDS writes and any scalar load: counted from zero)
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) lds_read128(a[s2], foff[s2], std::integral_constant<int, slot * UNIT_BYTES>{});
        static_for(std::make_integer_sequence<int, 8>{}, [&](auto sc) {
            constexpr int s2 = decltype(sc)::value;
            wait_lgkmcnt<(7 - s2 < 6 ? 7 - s2 : 6)>(a[s2]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s2], b[c * 8 + s2], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);  // (each MFMA right behind its own wait)
        });
        if (c == NCH - 1) {
            float mx = acc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[r]);
            if (__any(mx > sfloor)) {
                const int t = it / NCH;
                range_collect(hits, acc, t_begin + 32 * t + 4 * h, sfloor, th, t_end, t_base);
            }
        }
    };
    for (int it0 = 0; it0 < nunits; it0 += RANGE_STAGES) {
        static_for(std::make_integer_sequence<int, RANGE_STAGES>{}, [&](auto sc) {
            if (it0 + decltype(sc)::value < nunits) unit(sc, it0 + decltype(sc)::value);
        });
    }
    hits.finish();
}

// The canonical similarity chain of two rows in the kernels' layout (groups of eight components, [k0 k2 k4 k6 | k1 k3
// k5 k7]): fp32 fma over ascending components, the bits every dense k-NN route reports.
__device__ __forceinline__ float canonical_chain(const f32x4 *__restrict__ qp, const f32x4 *__restrict__ tp, int DP) {
    float c = 0.0f;
    for (int g = 0; g < DP / 8; ++g) {
        const f32x4 qe = qp[2 * g], qo = qp[2 * g + 1], te = tp[2 * g], to = tp[2 * g + 1];
        c = __builtin_fmaf(qe.x, te.x, c);
        c = __builtin_fmaf(qo.x, to.x, c);
        c = __builtin_fmaf(qe.y, te.y, c);
        c = __builtin_fmaf(qo.y, to.y, c);
        c = __builtin_fmaf(qe.z, te.z, c);
        c = __builtin_fmaf(qo.z, to.z, c);
        c = __builtin_fmaf(qe.w, te.w, c);
        c = __builtin_fmaf(qo.w, to.w, c);
    }
    return c;
}

// exact ranking of a collected range: one wave per query, keys staged in LDS
__global__ __launch_bounds__(256) void knn_rerank_long_kernel(
    const int *__restrict__ list, int count, const int *__restrict__ cnt, const int *__restrict__ cand,
    int K, const float *__restrict__ Qhat, const float *__restrict__ That, int DP, int t_base,
    int *__restrict__ idx_out, float *__restrict__ dist_out, int *__restrict__ counter,
    int *__restrict__ flagged, unsigned char *__restrict__ path) {
    __shared__ u64 keys[4][RANGE_CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= count) return;
    const int q = list[i];
    const int n = cnt[i];
    if (n > RANGE_CAP || n < K) {  // set too large (or, defensively, too small): exact kernel
        if (lane == 0) {
            flagged[atomicAdd(counter, 1)] = q;
            path[q] = FDR_PATH_RANGE_OVERFLOW;
        }
        return;
    }
    const f32x4 *qp = reinterpret_cast<const f32x4 *>(Qhat + (size_t)q * DP);
    for (int m = lane; m < n; m += 64) {
        const int tidx = cand[(size_t)i * RANGE_CAP + m];
        const f32x4 *tp = reinterpret_cast<const f32x4 *>(That + (size_t)(tidx - t_base) * DP);
        const float c = canonical_chain(qp, tp, DP);
        keys[wave][m] = ((u64)__float_as_uint(dist_from_sim(c)) << 32) | (unsigned)tidx;
    }
    u64 prev1 = 0, mine = 0;
    for (int r = 0; r < K; ++r) {
        u64 best = ~0ull;
        for (int m = lane; m < n; m += 64) {
            const u64 kv = keys[wave][m];
            if (kv + 1 > prev1 && kv < best) best = kv;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(best, off);
            best = o < best ? o : best;
        }
        prev1 = best + 1;
        if (lane == r) mine = best;
    }
    if (lane < K) {
        idx_out[(size_t)q * K + lane] = (int)(unsigned)(mine & 0xffffffffull);
        dist_out[(size_t)q * K + lane] = __uint_as_float((unsigned)(mine >> 32));
    }
}

__global__ __launch_bounds__(256) void gather_half_queries_kernel(const _Float16 *__restrict__ Qh,
                                                                  const float *__restrict__ theta_all,
                                                                  const int *__restrict__ list, int first,
                                                                  int count, int DP,
                                                                  _Float16 *__restrict__ Qc,
                                                                  float *__restrict__ theta_c,
                                                                  int *__restrict__ cnt) {
    const int i = blockIdx.x;
    if (i >= count) return;
    const int q = list[first + i];
    for (int c = threadIdx.x; c < DP; c += 256) Qc[(size_t)i * DP + c] = Qh[(size_t)q * DP + c];
    if (threadIdx.x == 0) {
        theta_c[i] = theta_all[q];
        cnt[i] = 0;
    }
}

// The neighbours of an all-zero query do not depend on the query: the all-zero targets at distance 0
// in index order, then every other target at distance 1 in index order.  One workgroup scans the
// zero flags for the first K rows of each kind (stops as soon as K zero rows are known).
__global__ __launch_bounds__(1024) void zero_answer_kernel(const unsigned *__restrict__ tzbits, int nt,
                                                           int t_base, int K, int *__restrict__ zidx,
                                                           float *__restrict__ zdist) {
    __shared__ int wz[16], wnz[16];
    __shared__ int zlist[FDR_MAX_K], nzlist[FDR_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nwords = (nt + 31) >> 5;
    int zc = 0, nzc = 0;  // found so far (uniform)
    for (int base = 0; base < nwords && zc < K; base += 1024) {  // 32768 rows per pass
        const int w = base + tid;
        unsigned zb = 0, nzb = 0;
        if (w < nwords) {
            const int rows = min(32, nt - 32 * w);
            const unsigned valid = rows == 32 ? ~0u : (1u << rows) - 1u;
            zb = tzbits[w] & valid;
            nzb = valid & ~zb;
        }
        const int z = __popc(zb), nz = __popc(nzb);
        int sz = z, snz = nz;  // inclusive scans over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int a = __shfl_up(sz, off), c = __shfl_up(snz, off);
            if (lane >= off) {
                sz += a;
                snz += c;
            }
        }
        if (lane == 63) {
            wz[wave] = sz;
            wnz[wave] = snz;
        }
        __syncthreads();
        int pz = zc + sz - z, pnz = nzc + snz - nz, tz = 0, tnz = 0;
        for (int w2 = 0; w2 < 16; ++w2) {
            if (w2 < wave) {
                pz += wz[w2];
                pnz += wnz[w2];
            }
            tz += wz[w2];
            tnz += wnz[w2];
        }
        for (unsigned m = zb; m && pz < K; m &= m - 1) zlist[pz++] = 32 * w + __ffs(m) - 1;
        for (unsigned m = nzb; m && pnz < K; m &= m - 1) nzlist[pnz++] = 32 * w + __ffs(m) - 1;
        zc += tz;
        nzc += tnz;
        __syncthreads();
    }
    if (zc > K) zc = K;
    if (tid < K) {
        const bool from_zero = tid < zc;
        zidx[tid] = t_base + (from_zero ? zlist[tid] : nzlist[tid - zc]);
        zdist[tid] = from_zero ? 0.0f : 1.0f;
    }
}

// (launched before the host knows how many all-zero queries there are: the count is read on the device;
// they are the last counter[1] entries of `flagged`, which has nq slots)
__global__ __launch_bounds__(256) void scatter_zero_answer_kernel(const int *__restrict__ zidx,
                                                                  const float *__restrict__ zdist,
                                                                  const int *__restrict__ flagged, int nq,
                                                                  const int *__restrict__ counter, int K,
                                                                  int *__restrict__ idx_out,
                                                                  float *__restrict__ dist_out) {
    const int count = counter[1];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)count * K) return;
    const int i = (int)(t / K), e = (int)(t - (long long)i * K);
    const int q = flagged[nq - count + i];
    idx_out[(size_t)q * K + e] = zidx[e];
    dist_out[(size_t)q * K + e] = zdist[e];
}

__global__ __launch_bounds__(256) void gather_queries_kernel(const float *__restrict__ Qhat,
                                                             const unsigned char *__restrict__ qzero,
                                                             const int *__restrict__ list, int first,
                                                             int count, int DP, float *__restrict__ Qc,
                                                             unsigned char *__restrict__ qzc) {
    const int i = blockIdx.x;  // one block per flagged query
    if (i >= count) return;
    const int q = list[first + i];
    for (int c = threadIdx.x; c < DP; c += 256) Qc[(size_t)i * DP + c] = Qhat[(size_t)q * DP + c];
    if (threadIdx.x == 0) qzc[i] = qzero[q];
}

__global__ __launch_bounds__(256) void scatter_results_kernel(const int *__restrict__ idxc,
                                                              const float *__restrict__ distc,
                                                              const int *__restrict__ list, int first,
                                                              int count, int K, int *__restrict__ idx_out,
                                                              float *__restrict__ dist_out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count * K) return;
    const int i = t / K, e = t - i * K;
    const int q = list[first + i];
    idx_out[(size_t)q * K + e] = idxc[t];
    dist_out[(size_t)q * K + e] = distc[t];
}

