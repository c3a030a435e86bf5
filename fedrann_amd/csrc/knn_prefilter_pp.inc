// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit), not compiled on its own.
// ------------------------------------------------------------------------------------------
// P1 for the shapes that need 256 registers (d <= 256 with K' > 32, d <= 512): the candidate pass in two
// alternating phases -- "ping-pong".
//
// What was measured on the round-3 kernel for these shapes (s_memtime stamps per stage, eight waves = two per SIMD,
// one workgroup per CU, a barrier per stage; devtools: -DFDR_STAMPS):
//     waves 0-3 (the older of each SIMD's pair): LDS-DMA issue 463, MFMAs + scoring 3065, waiting at the barrier 1928
//     waves 4-7 (the younger):                   LDS-DMA issue 960, MFMAs + scoring 4271, waiting at the barrier  140
// of a 5560-cycle stage whose 128 MFMAs per SIMD need 4096 (matrix pipe 73 % busy, at 2.37 GHz: not the clock).
// The SIMD serves the older wave first: it runs ahead, finishes its 64 MFMAs early and parks at the barrier while
// the younger finishes ALONE -- and a wave alone cannot keep the pipe fed, because its own LDS-DMA issue (60-180
// cycles a piece) and its score (the tile's last MFMA is 64 cycles of latency away) sit in the same instruction
// stream as its MFMAs.  Spreading the DMA pieces or deferring the score inside the one stream did not help (1 %).
//
// So the two waves of a SIMD take turns, and each turn is pure:
//     phase A: waves 0-3 issue the stage's 8 U MFMAs back to back (fragments streamed from LDS D k-steps ahead, nothing
//              else in the stream) into one accumulator set PER TILE of the stage;
//              waves 4-7 meanwhile score the tiles of THEIR previous turn (hot: ten integer maxima and a compare per
//              tile; cold: the register lists), issue their LDS-DMA pieces of the next stage, exchange bounds;
//     barrier; phase B: the roles swap; barrier.
// The pipe always has exactly one wave feeding it at the bare MFMA rate, and every vector instruction of the other
// wave issues in the 24 of 32 cycles an MFMA leaves the SIMD's issue port free.  A stage's TPS tiles keep their
// accumulators until the wave's next turn (TPS x 16 registers instead of 16).
// Rows are offered to a query's list in ascending scan order as before (tiles of a stage in order, stages in
// order): the exactness arguments of knn_prefilter.inc hold unchanged, and so does every result bit.
// ------------------------------------------------------------------------------------------
template <int DP, int U, int LH>
__global__ __launch_bounds__(512, 2) void knn_prefilter_pp_kernel(
    const _Float16 *__restrict__ Qh, int nq, const _Float16 *__restrict__ Th, int nt, int t_base,
    SegBounds segs, int K, int nq_pad, u64 *__restrict__ partial, unsigned *__restrict__ tau_shared,
    int ib, int item_base, int nqb, OrderArgs ord FDR_DBG_PARAM) {
#ifndef FDR_DEV
    constexpr int dbg = 0;
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NW = 8, QW = 32 * NW;
    constexpr int NCH = DP / 128;   // 128-component chunks (= units) per tile
    constexpr int TPS = U / NCH;    // tiles per stage
    static_assert(U % NCH == 0 && TPS >= 1, "a stage holds whole tiles");
    constexpr int UNIT_BYTES = 32 * 256, STAGE_BYTES = U * UNIT_BYTES, ROW_BYTES = DP * 2;
    constexpr int KS = 8 * U;       // k-steps (MFMAs) per stage and wave
    // fragments requested ahead / fragment registers (d <= 512 with 2 x 32-key lists: 128 query + 33 list registers leave
    // room for two fragments ahead and one tile's accumulators)
    constexpr int D = (DP == 512 && LH == 32) ? 2 : 4, R = D + 1;
    const int item = item_base + (int)blockIdx.x;
    const int seg = item / nqb, qb = item - seg * nqb;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;  // (waves w and w + 4 share a SIMD: a workgroup's waves are dealt to the SIMDs cyclically)
    const int j = lane & 31, h = lane >> 5;
    const int qg0 = qb * QW + wave * 32 + j;

    f16x8 b[NCH * 8];  // B fragments: chunk c, k-step s covers components 128c + 16s + 8h .. + 7
    {
        const f16x8 *qp = reinterpret_cast<const f16x8 *>(Qh + (size_t)(qg0 < nq ? qg0 : nq - 1) * DP);
#pragma unroll
        for (int i = 0; i < NCH * 8; ++i) b[i] = qp[2 * i + h];
    }
    // quantisation grid and the list (see knn_prefilter_kernel: the same state, one query set per wave)
    // (A COPY of that kernel's list code, on purpose: as one struct used by both kernels it cost the one-stream shapes
    // registers and scratch -- docs/experiments.md A-21.  A fix to share / rethreshold / flush / offer / the write-out
    // here must be made there too.)
    const int qbits = min(20, 32 - ib);
    const unsigned QM1 = (1u << qbits) - 2u;
    const float qscale = (float)QM1, qinv = 1.0f / qscale;
    const int nlive = (K - h + 1) >> 1, dead = LH - nlive;
    RegList<LH> L;
#pragma unroll
    for (int e = 0; e < LH; ++e) L.v[e] = e < dead ? 0u : PK_EMPTY;
    L.pmax = PK_EMPTY;
    unsigned flim;
    int cthr;
    auto share = [&]() {
        unsigned *slot = tau_shared + qg0;
        const unsigned tk = max(L.v[LH - 1], L.pmax);
        const unsigned mine = tk == PK_EMPTY ? 0x7F800000u : (tk >> ib);
        unsigned seen = mine;
        if (h == 0) {
            const unsigned old = mine <= QM1
                                     ? __hip_atomic_fetch_min(slot, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                     : __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            seen = min(old, mine);
        }
        const unsigned ps = partner32(seen, h);
        flim = min(h ? ps : seen, QM1 + 1);
    };
    auto rethreshold = [&]() -> int {
        const unsigned tk = max(L.v[LH - 1], L.pmax);
        const unsigned oq = tk >> ib;
        const unsigned lim = tk == PK_EMPTY ? flim : min(oq - 1u, flim);  // (oq == 0: wraps, handled below)
        int th = lim >= QM1 ? (int)0x80000000u : __float_as_int(((float)(QM1 - lim) - 0.75f) * qinv) + 1;
        if (tk != PK_EMPTY && oq == 0u) th = 0x7fffffff;
        return th;
    };
    share();
    cthr = rethreshold();
    if (dbg & 16) cthr = 0x7fffffff;

    const int t_begin = segs.b[seg];
    const int t_end = min(nt, segs.b[seg + 1]);
    const int ntiles = (t_end - t_begin + 31) >> 5;
    const int nstages = (ntiles + TPS - 1) / TPS;  // (a last, partly filled stage runs in full on clamped rows; its surplus tiles are not scored)

    // LDS-DMA through a buffer descriptor: piece p = wave + 8 u is unit u of the stage, rows 4 wave .. + 3 of it, 16 lanes
    // per row; the 16-byte slot a lane fetches is XOR-swizzled with the row.  One loop-invariant (row, slot) pair per
    // lane; rows past the segment end are clamped to its last row (and masked when the tile is scored).
    const char *seg_base = reinterpret_cast<const char *>(Th + (size_t)t_begin * DP);
    const unsigned last_row_off = (unsigned)(t_end - 1 - t_begin) * ROW_BYTES;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(seg_base), 0, (int)((unsigned)(t_end - t_begin) * ROW_BYTES), 0x00020000);
    const unsigned wrow = (unsigned)(4 * wave + (lane >> 4));
    const unsigned wvrow = wrow * ROW_BYTES;
    const unsigned wvslot = (((unsigned)lane & 15u) ^ (wrow & 15u)) * 16u;
    constexpr unsigned STAGE_SRC_BYTES = (unsigned)(32 * TPS) * ROW_BYTES;
    auto issue_stage = [&](const int par, const int stage) __attribute__((always_inline)) {  // this wave's U pieces of a stage
        const unsigned stage_off = (unsigned)stage * STAGE_SRC_BYTES;
        static_for(std::make_integer_sequence<int, U>{}, [&](auto u_c) {
            constexpr int u = decltype(u_c)::value;
            constexpr unsigned row_c = (unsigned)(32 * (u / NCH)) * ROW_BYTES;
            unsigned vrow = wvrow + stage_off;
            asm volatile("" : "+v"(vrow));  // (opaque: otherwise hipcc keeps wvrow + row_c of every piece in a register of its own)
            const unsigned vo = min(vrow + row_c, last_row_off) + wvslot;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsrc, (__attribute__((address_space(3))) void *)(smem + par * STAGE_BYTES + (wave + 8 * u) * 1024), 16,
                (int)vo, (u % NCH) * 256, 0, 0);
        });
    };

    // the cold path: a two-entry candidate queue per lane, batched insertion rounds (knn_prefilter_kernel)
    unsigned q0 = PK_EMPTY, q1 = PK_EMPTY;
    auto flush = [&]() {
        const bool dbgc = (dbg & 2) != 0;
        while (__any(q0 != PK_EMPTY)) {
            DBG_COUNT(4);
            const unsigned took = reglist_round<LH>(L, q0, h);
            if (q0 == took) {
                q0 = q1;
                q1 = PK_EMPTY;
            }
        }
    };
    auto offer = [&](const f32x16 &a, const int (&g)[4], int lrow, int nvalid) {
        const bool dbgc = (dbg & 2) != 0;
        DBG_COUNT(1);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            if (!__any(g[q4] >= cthr)) continue;
            DBG_COUNT(2);
#pragma unroll
            for (int r = 4 * q4; r < 4 * q4 + 4; ++r) {
                const int roff = (r & 3) + 8 * (r >> 2);
                const bool pass = __float_as_int(a[r]) >= cthr && roff + 4 * h < nvalid;
                if (!__any(pass)) continue;
                unsigned cand = PK_EMPTY;
                if (pass) {
                    const float sc = fminf(fmaxf(a[r], 0.0f), 1.0f);
                    const unsigned qd = QM1 - (unsigned)__builtin_rintf(sc * qscale);
                    if (qd <= flim) cand = (qd << ib) | (unsigned)(lrow + roff);
                }
                DBG_COUNT(3);
                if (__any(cand != PK_EMPTY && q1 != PK_EMPTY)) flush();  // some lane's queue is full
                q1 = (q0 != PK_EMPTY && q1 == PK_EMPTY) ? cand : q1;
                q0 = q0 == PK_EMPTY ? cand : q0;
            }
        }
    };
    // the row-group maxima of a finished tile, as integers (a similarity's bit pattern orders like its value)
    auto group_maxima = [&](const f32x16 &av, int (&g)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
            g[q4] = max(max(max(__float_as_int(av[4 * q4]), __float_as_int(av[4 * q4 + 1])),
                            __float_as_int(av[4 * q4 + 2])),
                        __float_as_int(av[4 * q4 + 3]));
    };

    unsigned fa[8];
    fragment_addresses(fa, smem, j, h);
    f32x16 acc[TPS];
#pragma unroll
    for (int t = 0; t < TPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    f16x8 fr[R];

    // a turn at the matrix pipe: the stage's KS MFMAs, nothing else in the stream.  `primed`: the first D fragment reads
    // were issued before the barrier that opened the turn (the stage's rows were known to be complete by then).
    // (the fragment addresses fa always point into the CURRENT stage's ring slot: they move at the end of every stage,
    // so the stage body needs no compile-time parity and the loop has ONE body per group)
    auto rd = [&](auto s_c) __attribute__((always_inline)) {
        constexpr int s = decltype(s_c)::value;
        lds_read128(fr[s % R], fa[s % 8], std::integral_constant<int, (s / 8) * UNIT_BYTES>{});
    };
    auto prime = [&]() __attribute__((always_inline)) {
        static_for(std::make_integer_sequence<int, D>{}, [&](auto s_c) { rd(s_c); });
    };
    auto mfma_turn = [&]() __attribute__((always_inline)) {
        static_for(std::make_integer_sequence<int, KS>{}, [&](auto s_c) {
            constexpr int s = decltype(s_c)::value;
            constexpr int uu = s / 8, s8 = s % 8, c = uu % NCH, tl = uu / NCH;
            if constexpr (s + D < KS) rd(std::integral_constant<int, s + D>{});
            wait_lgkmcnt<(KS - 1 - s < D ? KS - 1 - s : D)>(fr[s % R]);
            __builtin_amdgcn_sched_barrier(0);
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[s % R], b[c * 8 + s8],
                                                             (c == 0 && s8 == 0) ? f32x16{} : acc[tl], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    // the other turn: score the tiles of stage `it` (accumulated in this wave's last turn at the pipe), exchange bounds now
    // and then.  Hot: per tile ten integer maxima and one compare, which only marks the tiles that hold a candidate; cold:
    // the marked tiles one by one through ONE copy of the list code (the tile's accumulators are moved to `cur`: sixteen
    // moves per cold tile instead of TPS inlined copies of offer() and its flush loops per turn -- the kernel's code size,
    // and with it the instruction cache's share of a cold tile, no longer grows with the tiles per stage).  The marks use
    // the threshold as it was when the turn began: looser than after the first insertions, never wrong (offer() tests
    // every row against the current one).
    auto score_turn = [&](const int it) __attribute__((always_inline)) {
        unsigned cold = 0u;  // (wave-uniform)
#pragma unroll
        for (int tl = 0; tl < TPS; ++tl) {
            int g[4];
            group_maxima(acc[tl], g);
            const int mx = max(max(max(g[0], g[1]), g[2]), g[3]);
            const bool dbgc = (dbg & 2) != 0;
            DBG_COUNT(0);
            if (dbg & 1) {  // timing experiment: MFMA + fast path only
                if (mx == 0x7fffffff) cthr = mx;
            } else if (it * TPS + tl < ntiles && __any(mx >= cthr)) {
                cold |= 1u << tl;
            }
        }
        while (cold) {
            const int tl = __builtin_ctz(cold);
            cold &= cold - 1u;
            const int t = it * TPS + tl;
            int lrow = t * 32 + 4 * h;  // row - segment start of this lane's first row
            int nvalid = t_end - (t_begin + t * 32);
            int g[4];
            if constexpr (TPS == 1) {  // (one tile per stage: its accumulators as they stand)
                group_maxima(acc[0], g);
                offer(acc[0], g, lrow, nvalid);
            } else {
                f32x16 cur;
                static_for(std::make_integer_sequence<int, TPS>{}, [&](auto t_c) {
                    if (tl == decltype(t_c)::value) cur = acc[decltype(t_c)::value];
                });
                group_maxima(cur, g);
                offer(cur, g, lrow, nvalid);
            }
            cthr = rethreshold();
        }
        if ((it & FDR_SHARE_EVERY) == FDR_SHARE_EVERY) {
            flush();
            share();
            cthr = rethreshold();
            if (dbg & 16) cthr = 0x7fffffff;
        }
    };
    auto next_slot = [&](const int par) __attribute__((always_inline)) {  // the fragment addresses move to the other ring slot
        const unsigned delta = par ? (unsigned)(-STAGE_BYTES) : (unsigned)STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < 8; ++i) fa[i] += delta;
    };
    auto wait_dma_and_sync = [&]() __attribute__((always_inline)) {  // this wave's pieces have landed; then everyone's
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    // prologue: stage 0 by all waves (the builtin wait, unlike the asm one, also tells hipcc that the query fragments'
    // loads have returned: it would otherwise count vmcnt down in front of the first MFMAs of every turn)
    if (nstages > 0) issue_stage(0, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __builtin_amdgcn_s_barrier();

#ifdef FDR_STAMPS  // (development: phases 0 pipe turn, 1 LDS-DMA issue, 2 scoring, 3 / 4 waiting at the barrier after the pipe / the
                   // other turn, 5 stages, 6 other turns longer than a pipe turn's KS * 32 cycles; 32-bit sums of 32-bit stamps:
                   // a stamped build must not spill what the release build keeps in registers)
    unsigned stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool stamp_on = blockIdx.x == 0;
#endif
    // One stage = two phases.  Group 0 (waves 0-3): pipe in phase A, scoring + fetching in phase B.  Group 1 (waves 4-7):
    // scoring (its previous stage) + fetching in phase A, pipe in phase B.  A stage's rows (ring slot par) are complete
    // at its start; the pieces of stage it + 1 go to slot par ^ 1, which stage it - 1 left at the end of ITS phase B.
    if (grp == 0) {
        for (int it = 0; it < nstages; ++it) {
            const int par = it & 1;
            STAMP(t0);
            prime();
            mfma_turn();
            STAMP(t1);
            __builtin_amdgcn_s_barrier();  // ---- phase A | phase B (nothing of group 0's is in flight)
            STAMP(t2);
            if (it + 1 < nstages) issue_stage(par ^ 1, it + 1);
            STAMP(t3);
            score_turn(it);
            next_slot(par);
            STAMP(t4);
            wait_dma_and_sync();           // ---- stage it | stage it + 1
            STAMP(t5);
            STAMP_ADD(0, t0, t1); STAMP_ADD(3, t1, t2); STAMP_ADD(1, t2, t3); STAMP_ADD(2, t3, t4); STAMP_ADD(4, t4, t5);
#ifdef FDR_STAMPS
            if (stamp_on) { stamp_acc[5] += 1; stamp_acc[6] += (t4 - t2) > (unsigned)(KS * 32); }
#endif
        }
    } else {
        for (int it = 0; it < nstages; ++it) {
            const int par = it & 1;
            STAMP(t0);
            if (it + 1 < nstages) issue_stage(par ^ 1, it + 1);
            STAMP(t1);
            if (it > 0) score_turn(it - 1);
            prime();                       // (the stage was complete at its start: the first fragments are on their way)
            STAMP(t2);
            __builtin_amdgcn_s_barrier();  // ---- phase A | phase B (this wave's pieces of stage it + 1 stay in flight)
            STAMP(t3);
            mfma_turn();
            next_slot(par);
            STAMP(t4);
            wait_dma_and_sync();           // ---- stage it | stage it + 1
            STAMP(t5);
            STAMP_ADD(1, t0, t1); STAMP_ADD(2, t1, t2); STAMP_ADD(4, t2, t3); STAMP_ADD(0, t3, t4); STAMP_ADD(3, t4, t5);
#ifdef FDR_STAMPS
            if (stamp_on) { stamp_acc[5] += 1; stamp_acc[6] += (t2 - t0) > (unsigned)(KS * 32); }
#endif
        }
    }
    if (grp == 1 && nstages > 0) score_turn(nstages - 1);  // group 1's last turn at the pipe
    flush();
#ifdef FDR_STAMPS
    if (stamp_on && lane == 0)
        for (int ph = 0; ph < 8; ++ph) atomicAdd(&g_stamps[wave][ph], stamp_acc[ph]);
#endif

    // write-out (as knn_prefilter_kernel): the list's two sorted halves, rows back in the targets' own numbers
    const unsigned imask = (1u << ib) - 1u;
    size_t qrow = (size_t)qb * QW + wave * 32 + j;
    if (ord.perm_q) {
        if (qrow >= (size_t)nq) return;
        qrow = (size_t)ord.perm_q[qrow];
    }
    u64 *out = partial + ((size_t)seg * nq_pad + qrow) * K + (h ? (K + 1) >> 1 : 0);
#pragma unroll
    for (int e = 0; e < LH; ++e) {
        if (e >= dead) {
            const unsigned kv = L.v[e];
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

// ---- the range pass in the same two phases ---------------------------------------------------------------------
// knn_range_kernel's job (knn_prefilter.inc: collect {targets with d~ <= theta} for the plateau queries; no top-k state)
// on the ping-pong skeleton above: a rank of config 4 sends 99 k of its 916 k queries through this pass (76 of 637 ms at
// 0.66 of the fp16 peak with one-unit stages and a barrier per eight MFMAs), a rank of config 5 12 k (58 ms).  Here a
// stage is eight units, a wave's turn at the pipe 64 MFMAs, and the other turn tests the stage's tiles against the
// query's similarity floor (one max tree per tile) and gathers the rare hits in the lane's LDS buffer.
// (The skeleton -- descriptor, issue_stage, rd / prime / mfma_turn, next_slot, the two groups' loops -- is a copy of
// knn_prefilter_pp_kernel's with another score_turn: one function template for both changed both kernels' registers and
// scratch, docs/experiments.md A-21.  This copy clamps an empty segment's descriptor and last row; the candidate pass's
// work items are the plan's segments, which each hold at least one row.)
// Grid: x = query block (256 queries), y = target segment.
template <int DP, int U, class Sink = RangeHits<512>>
__global__ __launch_bounds__(512, 2) void knn_range_pp_kernel(
    const _Float16 *__restrict__ Qh, const float *__restrict__ theta, int nq,
    const _Float16 *__restrict__ Th, int nt, int t_base, SegBounds segs, const typename Sink::Out out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NW = 8, QW = 32 * NW;
    constexpr int NCH = DP / 128, TPS = U / NCH;
    static_assert(U % NCH == 0 && TPS >= 1, "a stage holds whole tiles");
    constexpr int UNIT_BYTES = 32 * 256, STAGE_BYTES = U * UNIT_BYTES, ROW_BYTES = DP * 2;
    constexpr int KS = 8 * U, D = 4, R = D + 1;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int j = lane & 31, h = lane >> 5;
    const int qg = blockIdx.x * QW + wave * 32 + j;
    const bool live = qg < nq;
    const int qrow = live ? qg : nq - 1;
    const float th = live ? theta[qrow] : -1.0f;                             // admit d~ <= th
    const float sfloor = live ? (1.0f - th) - 3.0e-7f : __builtin_inff();    // conservative similarity form

    f16x8 b[NCH * 8];
    {
        const f16x8 *qp = reinterpret_cast<const f16x8 *>(Qh + (size_t)qrow * DP);
#pragma unroll
        for (int i = 0; i < NCH * 8; ++i) b[i] = qp[2 * i + h];
    }
    const int t_begin = segs.b[blockIdx.y];
    const int t_end = min(nt, segs.b[blockIdx.y + 1]);
    const int ntiles = (t_end - t_begin + 31) >> 5;
    const int nstages = (ntiles + TPS - 1) / TPS;

    const char *seg_base = reinterpret_cast<const char *>(Th + (size_t)t_begin * DP);
    const unsigned last_row_off = (unsigned)(max(t_end - 1 - t_begin, 0)) * ROW_BYTES;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(seg_base), 0, (int)((unsigned)max(t_end - t_begin, 0) * ROW_BYTES), 0x00020000);
    const unsigned wrow = (unsigned)(4 * wave + (lane >> 4));
    const unsigned wvrow = wrow * ROW_BYTES;
    const unsigned wvslot = (((unsigned)lane & 15u) ^ (wrow & 15u)) * 16u;
    constexpr unsigned STAGE_SRC_BYTES = (unsigned)(32 * TPS) * ROW_BYTES;
    auto issue_stage = [&](const int par, const int stage) __attribute__((always_inline)) {
        const unsigned stage_off = (unsigned)stage * STAGE_SRC_BYTES;
        static_for(std::make_integer_sequence<int, U>{}, [&](auto u_c) {
            constexpr int u = decltype(u_c)::value;
            constexpr unsigned row_c = (unsigned)(32 * (u / NCH)) * ROW_BYTES;
            unsigned vrow = wvrow + stage_off;
            asm volatile("" : "+v"(vrow));
            const unsigned vo = min(vrow + row_c, last_row_off) + wvslot;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsrc, (__attribute__((address_space(3))) void *)(smem + par * STAGE_BYTES + (wave + 8 * u) * 1024), 16,
                (int)vo, (u % NCH) * 256, 0, 0);
        });
    };
    Sink hits = Sink::make(reinterpret_cast<int *>(smem + 2 * STAGE_BYTES), out, qg, tid);  // (the lane buffers: behind the ring)
    unsigned fa[8];
    fragment_addresses(fa, smem, j, h);
    f32x16 acc[TPS];
#pragma unroll
    for (int t = 0; t < TPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    f16x8 fr[R];
    auto rd = [&](auto s_c) __attribute__((always_inline)) {
        constexpr int s = decltype(s_c)::value;
        lds_read128(fr[s % R], fa[s % 8], std::integral_constant<int, (s / 8) * UNIT_BYTES>{});
    };
    auto prime = [&]() __attribute__((always_inline)) {
        static_for(std::make_integer_sequence<int, D>{}, [&](auto s_c) { rd(s_c); });
    };
    auto mfma_turn = [&]() __attribute__((always_inline)) {
        static_for(std::make_integer_sequence<int, KS>{}, [&](auto s_c) {
            constexpr int s = decltype(s_c)::value;
            constexpr int uu = s / 8, s8 = s % 8, c = uu % NCH, tl = uu / NCH;
            if constexpr (s + D < KS) rd(std::integral_constant<int, s + D>{});
            wait_lgkmcnt<(KS - 1 - s < D ? KS - 1 - s : D)>(fr[s % R]);
            __builtin_amdgcn_sched_barrier(0);
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[s % R], b[c * 8 + s8],
                                                             (c == 0 && s8 == 0) ? f32x16{} : acc[tl], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    auto score_turn = [&](const int it) __attribute__((always_inline)) {
        unsigned cold = 0u;
#pragma unroll
        for (int tl = 0; tl < TPS; ++tl) {
            float mx = acc[tl][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[tl][r]);
            if (it * TPS + tl < ntiles && __any(mx > sfloor)) cold |= 1u << tl;
        }
        while (cold) {
            const int tl = __builtin_ctz(cold);
            cold &= cold - 1u;
            f32x16 cur;
            static_for(std::make_integer_sequence<int, TPS>{}, [&](auto t_c) {
                if (tl == decltype(t_c)::value) cur = acc[decltype(t_c)::value];
            });
            range_collect(hits, cur, t_begin + 32 * (it * TPS + tl) + 4 * h, sfloor, th, t_end, t_base);
        }
    };
    auto next_slot = [&](const int par) __attribute__((always_inline)) {
        const unsigned delta = par ? (unsigned)(-STAGE_BYTES) : (unsigned)STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < 8; ++i) fa[i] += delta;
    };
    auto wait_dma_and_sync = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };
    if (nstages > 0) issue_stage(0, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) (and the query fragments, as hipcc sees it)
    __builtin_amdgcn_s_barrier();
    if (grp == 0) {
        for (int it = 0; it < nstages; ++it) {
            const int par = it & 1;
            prime();
            mfma_turn();
            __builtin_amdgcn_s_barrier();
            if (it + 1 < nstages) issue_stage(par ^ 1, it + 1);
            score_turn(it);
            next_slot(par);
            wait_dma_and_sync();
        }
    } else {
        for (int it = 0; it < nstages; ++it) {
            const int par = it & 1;
            if (it + 1 < nstages) issue_stage(par ^ 1, it + 1);
            if (it > 0) score_turn(it - 1);
            prime();
            __builtin_amdgcn_s_barrier();
            mfma_turn();
            next_slot(par);
            wait_dma_and_sync();
        }
        if (nstages > 0) score_turn(nstages - 1);
    }
    if (live) hits.finish();
}
