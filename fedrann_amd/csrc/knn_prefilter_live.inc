// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit), not compiled on its own.
// ------------------------------------------------------------------------------------------
// Live-chunk candidate pass for d <= 128, K' <= 32 (DESIGN.md section 6, docs/experiments.md A-22).
//
// A normalised row has 4-6 non-zero components of 128, the rows are scanned in (non-empty chunks, chunk mask) order
// (knn_order.inc), so the 256 consecutive queries of a workgroup share one chunk mask, or nearly: at 1 M reads 0.555 of
// the pass's k-steps have a query chunk that is non-zero in SOME query of the block.  The other k-steps add exactly +0
// to every accumulator.  knn_prefilter_live_kernel<NL> is knn_prefilter_kernel<128, 1, 8, 4, 4, 16, true> -- eight
// waves, four-tile stages, two MFMA chains, staggered halves, the same lists, bound exchange and write-back -- with the
// block's NL live chunk ids fixed BEFORE the stage loop: the loop holds no mask, no branch and no scalar instruction
// more than the dense kernel's, only fewer LDS-DMA pieces, ds_read_b128 and MFMAs (NL instead of 8 per tile) and 4 NL
// instead of 32 query-fragment registers.  The kept k-steps run in the same ascending order onto the same inline-zero
// start, so the similarities are the dense pass's bit for bit.
//
// It streams the BLOCKED ordered copy of the targets (to_half_blocked_kernel): [tile of 32 rows][chunk 0..7][32 rows]
// [16 components], 1 KiB per (tile, chunk) = one LDS-DMA piece.  DMA lane i fetches the 16 bytes of row i & 31, half
// i >> 5 of the piece, so that in LDS the piece is [half][row] and fragment lane (j, h) reads the 16 bytes at
// (32 h + j) * 16 = lane * 16: one address register for every read, no bank conflict.
// ------------------------------------------------------------------------------------------

// chunk masks of the query blocks: bit c of masks[b] <=> chunk c is non-empty in some of the ordered queries
// [256 b, 256 b + 256).  keys_s = the sorted keys of row_chunk_keys_kernel (low word: the row's mask).  One wave a block.
__global__ __launch_bounds__(64) void live_block_masks_kernel(const u64 *__restrict__ keys_s, int nq,
                                                              unsigned *__restrict__ masks) {
    const int b = blockIdx.x, lane = threadIdx.x;
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = b * 256 + i * 64 + lane;
        if (r < nq) m |= (unsigned)keys_s[r] & 0xffu;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m |= __shfl_xor(m, off);
    if (lane == 0) masks[b] = m;
}

// Stage skipping.  The targets are scanned in (live chunks, mask) order, so a stage -- four tiles = 128 ordered rows
// counted from its segment's first row, as the kernel below cuts them -- holds one mask or few.  Where the OR of its
// rows' masks shares no chunk with the query block's mask, every similarity of the stage is exactly 0: it can enter no
// list that is full, and a work item need not visit it.  Stage 0 of a segment is always visited: it fills a list that
// nothing else fills with d~ = 1 entries, as the whole scan did.
//
// smask[live_stage_row(segment) + stage] = the OR of the masks of the stage's rows (rows from the segment's end on, or
// from nt on, contribute nothing).  keys_s = the TARGETS' sorted keys.  One wave a stage: grid (stages of the longest
// segment, segments).
__global__ __launch_bounds__(64) void live_stage_masks_kernel(const u64 *__restrict__ keys_s, int nt, SegBounds segs,
                                                              uint8_t *__restrict__ smask) {
    const int seg = blockIdx.y, stage = blockIdx.x, lane = threadIdx.x;
    const int t_begin = segs.b[seg], t_end = min(nt, segs.b[seg + 1]);
    const int r0 = t_begin + stage * 128;
    if (r0 >= t_end) return;
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = r0 + i * 64 + lane;
        if (r < t_end) m |= (unsigned)keys_s[r] & 0xffu;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m |= __shfl_xor(m, off);
    if (lane == 0) smask[live_stage_row(t_begin, seg) + stage] = (uint8_t)m;
}

// The lists: for segment blockIdx.y and block mask value v = blockIdx.x, ascending, stage 0 and every stage whose mask
// shares a chunk with v (all != 0: every stage -- the switch's off position), and lens[segment * 256 + v] = their
// number.  One wave a list, 64 stages a step: a lane's entry goes behind those of the lanes below it.
__global__ __launch_bounds__(64) void live_stage_lists_kernel(const uint8_t *__restrict__ smask, int nt, SegBounds segs,
                                                              int all, uint16_t *__restrict__ lists,
                                                              int *__restrict__ lens) {
    const int seg = blockIdx.y, lane = threadIdx.x;
    const unsigned v = blockIdx.x;
    const int t_begin = segs.b[seg], t_end = min(nt, segs.b[seg + 1]);
    const int nstages = t_end > t_begin ? (t_end - t_begin + 127) >> 7 : 0;
    const size_t row = (size_t)live_stage_row(t_begin, seg);
    const uint8_t *sm = smask + row;
    uint16_t *out = lists + row * 256 + (size_t)v * live_list_stride(nstages);
    int count = 0;
    for (int s0 = 0; s0 < nstages; s0 += 64) {
        const int s = s0 + lane;
        const bool keep = s < nstages && (s == 0 || all != 0 || (sm[s] & v) != 0u);
        const unsigned long long kept = __ballot(keep);
        if (keep) out[count + __popcll(kept & ((1ull << lane) - 1ull))] = (uint16_t)s;
        count += __popcll(kept);
    }
    if (lane == 0) lens[seg * 256 + (int)v] = count;
}

// Ehat fp32 [n, 128] (k0 k2 k4 k6 k1 k3 k5 k7 inside each group of 8), rows in the order `perm` -> the blocked fp16 copy
// of `tiles` tiles (rows from n on: zeros).  One thread per 8 components.
__global__ __launch_bounds__(256) void to_half_blocked_kernel(const float *__restrict__ Ehat,
                                                              const int *__restrict__ perm, int n, long long n_groups,
                                                              _Float16 *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_groups) return;
    const long long i = t >> 4;  // ordered row
    const int g = (int)(t & 15);   // its group of 8 components: chunk g >> 1, half g & 1
    f16x8 h;
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = (_Float16)0.0f;
    if (i < n) {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(Ehat) + ((size_t)perm[i] * 16 + g) * 2;
        const f32x4 e = src[0], o = src[1];
        h[0] = (_Float16)e.x; h[1] = (_Float16)o.x; h[2] = (_Float16)e.y; h[3] = (_Float16)o.y;
        h[4] = (_Float16)e.z; h[5] = (_Float16)o.z; h[6] = (_Float16)e.w; h[7] = (_Float16)o.w;
    }
    // 16-byte slot: ((tile * 8 + chunk) * 32 + row in tile) * 2 + half
    const size_t slot = ((((size_t)(i >> 5) * 8 + (size_t)(g >> 1)) * 32 + (size_t)(i & 31)) << 1) + (size_t)(g & 1);
    reinterpret_cast<f16x8 *>(out)[slot] = h;
}

// The dense group's query blocks side by side: block i of the gathered arrays = ordered block blocks[i] -- its fp16 rows,
// its rows' own numbers and its bound words (still at their initial value: the pass has not started).  The shipped
// kernel scans a RANGE of blocks; gathered, the blocks of seven or eight live chunks, scattered over the order wherever
// 256 rows straddle two masks, are one range and run in full launches.  One workgroup a block, 16 lanes a row.
__global__ __launch_bounds__(256) void live_gather_dense_kernel(const _Float16 *__restrict__ hq, const int *__restrict__ perm_q,
                                                                const unsigned *__restrict__ tau, int nq,
                                                                const int *__restrict__ blocks, _Float16 *__restrict__ out_q,
                                                                int *__restrict__ out_perm, unsigned *__restrict__ out_tau) {
    const int b = blocks[blockIdx.x];
    const int sub = threadIdx.x & 15;
    for (int r = threadIdx.x >> 4; r < 256; r += 16) {
        const int src = b * 256 + r, dst = blockIdx.x * 256 + r;
        if (src >= nq) {  // (the last block of the order may be short; it is the group's last as well)
            if (sub == 0) out_tau[dst] = 0x7F800000u;
            continue;
        }
        reinterpret_cast<f16x8 *>(out_q)[(size_t)dst * 16 + sub] = reinterpret_cast<const f16x8 *>(hq)[(size_t)src * 16 + sub];
        if (sub == 0) {
            out_perm[dst] = perm_q[src];
            out_tau[dst] = tau[src];
        }
    }
}

// Work item = (target segment, query block of the launch's group), segment-major: item / nb is the segment,
// blocks[item % nb] the query block, live_ids[block] its NL chunk ids (ascending, four bits each; live_plan).
// (The list code -- share, rethreshold, flush, offer, score, the write-out -- is a THIRD copy of knn_prefilter_kernel's,
// beside knn_prefilter_pp_kernel's: a fix there must be made here too; docs/experiments.md A-21.)
template <int NL>
__global__ __launch_bounds__(512, 4) void knn_prefilter_live_kernel(
    const _Float16 *__restrict__ Qh, int nq, const _Float16 *__restrict__ Tb, int nt, int t_base, SegBounds segs, int K,
    int nq_pad, u64 *__restrict__ partial, unsigned *__restrict__ tau_shared, int ib, int item_base, int nb,
    const int *__restrict__ blocks, const unsigned *__restrict__ live_ids, OrderArgs ord,
    const unsigned *__restrict__ masks, const unsigned *__restrict__ lists, const int *__restrict__ lens) {
    static_assert(NL >= FDR_LIVE_MIN_NL && NL <= FDR_LIVE_MAX_NL, "instances NL = 2 .. 6");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int DP = 128, NW = 8, U = 4, LH = 16, QW = 32 * NW;
    constexpr int TILE_BYTES = 8 * 1024;            // a tile of the blocked copy: eight pieces
    constexpr int UNIT_BYTES = NL * 1024;           // ... of which a stage holds the NL live ones
    constexpr int STAGE_BYTES = U * UNIT_BYTES;
    constexpr int NPIECE = U * NL;                  // pieces per stage
    constexpr int PPW = (NPIECE + NW - 1) / NW;     // ... per wave (the last one only for waves < NPIECE - 8 (PPW - 1))
    const int item = item_base + (int)blockIdx.x;
    const int seg = item / nb;
    const int qb = __builtin_amdgcn_readfirstlane(blocks[item - seg * nb]);
    const unsigned ids = __builtin_amdgcn_readfirstlane(live_ids[qb]);
    const unsigned bmask = __builtin_amdgcn_readfirstlane(masks[qb]) & 0xffu;  // the block's own mask: its list

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ql0 = wave * 32 + j;
    const int qg0 = qb * QW + ql0;

    f16x8 b[NL];  // B fragments of the live chunks: chunk ids[s], components 16 ids[s] + 8 h .. + 7
    {
        const f16x8 *qp = reinterpret_cast<const f16x8 *>(Qh + (size_t)(qg0 < nq ? qg0 : nq - 1) * DP);
#pragma unroll
        for (int s = 0; s < NL; ++s) b[s] = qp[2 * (int)((ids >> (4 * s)) & 7u) + h];
    }
    const int qbits = min(20, 32 - ib);
    const unsigned QM1 = (1u << qbits) - 2u;
    const float qscale = (float)QM1, qinv = 1.0f / qscale;
    const int nlive = (K - h + 1) >> 1, dead = LH - nlive;  // live entries of this half
    RegList<LH> L;
    unsigned flim;  // cross-segment bound on qd (admits qd <= flim); QM1 + 1 = none
    int cthr;       // a similarity can enter only if its bit pattern, as a signed int, is >= cthr
#pragma unroll
    for (int e = 0; e < LH; ++e) L.v[e] = e < dead ? 0u : PK_EMPTY;
    L.pmax = PK_EMPTY;
    auto share = [&](RegList<LH> &Ln, unsigned &fl) {
        unsigned *slot = tau_shared + qg0;
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
    auto rethreshold = [&](const RegList<LH> &Ln, unsigned fl) -> int {  // (knn_prefilter_kernel: why it is what it is)
        const unsigned tk = max(Ln.v[LH - 1], Ln.pmax);
        const unsigned oq = tk >> ib;
        const unsigned lim = tk == PK_EMPTY ? fl : min(oq - 1u, fl);  // (oq == 0: wraps, handled below)
        int th = lim >= QM1 ? (int)0x80000000u : __float_as_int(((float)(QM1 - lim) - 0.75f) * qinv) + 1;
        if (tk != PK_EMPTY && oq == 0u) th = 0x7fffffff;
        return th;
    };
    share(L, flim);
    cthr = rethreshold(L, flim);

    const int t_begin = segs.b[seg];  // (a multiple of 32: whole tiles of the blocked copy)
    const int t_end = min(nt, segs.b[seg + 1]);
    const int nunits = (t_end - t_begin + 31) >> 5;  // tiles
    const int nstages = (nunits + U - 1) / U;
    // The stages this work item walks (live_stage_lists_kernel): nlist numbers, ascending, 16 bits each, from a word
    // boundary on.  entry(i) is a scalar load of the word that holds number min(i, nlist - 1); the loop keeps the number
    // of the stage it multiplies, of the one before (whose last pair the late half scores) and of the one it issues, and
    // asks for the next one an iteration ahead of its use.
    const int nlist = nstages > 0 ? min(lens[seg * 256 + (int)bmask], nstages) : 0;
    const unsigned *list = lists + (((size_t)live_stage_row(t_begin, seg) * 256 + (size_t)bmask * live_list_stride(nstages)) >> 1);
    auto entry = [&](int i) -> int {
        const int e = max(min(i, nlist - 1), 0);
        const unsigned w = __builtin_amdgcn_readfirstlane(list[e >> 1]);
        return min((int)((w >> (16 * (e & 1))) & 0xffffu), max(nstages - 1, 0));  // (never past the segment, whatever the table holds)
    };

    // LDS-DMA: piece p = wave + 8 u of a stage is live chunk p % NL of the stage's tile p / NL and lands at p KiB of the
    // stage.  Its source offset inside the stage's four tiles is loop-invariant (a scalar per piece); the stage advances
    // by four tiles.  Tiles past the segment's end are other segments' rows or the copy's padding: fetched, never scored.
    const char *seg_base = reinterpret_cast<const char *>(Tb) + (size_t)(t_begin >> 5) * TILE_BYTES;
    unsigned poff[PPW];
#pragma unroll
    for (int u = 0; u < PPW; ++u) {
        const int p = min(wave + NW * u, NPIECE - 1);
        const int tl = p / NL, s = p - tl * NL;
        poff[u] = (unsigned)(tl * TILE_BYTES) + ((ids >> (4 * s)) & 7u) * 1024u;
    }
    const unsigned soff = (unsigned)((lane & 31) * 32 + (lane >> 5) * 16);  // this lane's 16 bytes of a piece
    auto issue_stage = [&](auto par_c, int sn) {  // par = parity of the list position being issued, sn = its stage
        const unsigned stoff = (unsigned)sn * (unsigned)(U * TILE_BYTES);
        constexpr int par = decltype(par_c)::value;
        unsigned char *dst = smem + par * STAGE_BYTES;
        static_for(std::make_integer_sequence<int, PPW>{}, [&](auto u_c) {
            constexpr int u = decltype(u_c)::value;
            if (NW * (u + 1) <= NPIECE || wave < NPIECE - NW * u)  // (wave-uniform; a literal for every u but the last)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(seg_base + (soff + (poff[u] + stoff))),
                                                 (__attribute__((address_space(3))) void *)(dst + (wave + NW * u) * 1024),
                                                 16, 0, 0);
        });
    };
    int sprev = 0, scur = entry(0), snext = entry(1);
    if (nlist > 0) issue_stage(std::integral_constant<int, 0>{}, scur);
    __syncthreads();  // (hipcc drains the DMA before the barrier)

    unsigned q0 = PK_EMPTY, q1 = PK_EMPTY;  // two-entry candidate queue per lane (knn_prefilter_kernel)
    auto flush = [&](RegList<LH> &Ln, unsigned &a0, unsigned &a1) {
        while (__any(a0 != PK_EMPTY)) {
            const unsigned took = reglist_round<LH>(Ln, a0, h);  // the smaller head of the query's two lanes
            if (a0 == took) {
                a0 = a1;
                a1 = PK_EMPTY;
            }
        }
    };
    auto offer = [&](const f32x16 &a, const int (&g)[4], RegList<LH> &Ln, unsigned &a0, unsigned &a1,
                     const unsigned fl, const int th, int lrow, int nvalid) {
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            if (!__any(g[q4] >= th)) continue;
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
                if (__any(cand != PK_EMPTY && a1 != PK_EMPTY)) flush(Ln, a0, a1);  // some lane's queue is full
                a1 = (a0 != PK_EMPTY && a1 == PK_EMPTY) ? cand : a1;
                a0 = a0 == PK_EMPTY ? cand : a0;
            }
        }
    };
    unsigned fa = (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char *)smem + (unsigned)lane * 16u;
    asm volatile("" : "+v"(fa));

    f32x16 acc, accB;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = accB[r] = 0.f;

    auto score = [&](const f32x16 &av, int t) __attribute__((always_inline)) {
        int g[4];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
            g[q4] = max(max(max(__float_as_int(av[4 * q4]), __float_as_int(av[4 * q4 + 1])),
                            __float_as_int(av[4 * q4 + 2])),
                        __float_as_int(av[4 * q4 + 3]));
        const int mx = max(max(max(g[0], g[1]), g[2]), g[3]);
        if (__any(mx >= cthr)) {
            int lrow = t * 32 + 4 * h;  // row - segment start of this lane's first row
            int nvalid = t_end - (t_begin + t * 32);
            asm volatile("" : "+v"(lrow), "+s"(nvalid));  // keep the cold block's set-up cold
            offer(av, g, L, q0, q1, flim, cthr, lrow, nvalid);
            cthr = rethreshold(L, flim);
        }
    };
    constexpr int NP = U / 2;           // pairs of tiles per stage
    const bool late = wave >= NW / 2;  // staggered halves: waves 4 .. 7 score a pair of tiles one pair later
#ifdef FDR_STAMPS
    unsigned stamp_acc[6] = {0, 0, 0, 0, 0, 0};
    const bool stamp_on = blockIdx.x == 0;
#endif
    auto stage_body = [&](auto par_c, int it) {  // it = position in the list; stage scur is multiplied, snext issued
        constexpr int par = decltype(par_c)::value;
        STAMP(ts0);
        const int safter = entry(it + 2);
        if (it + 1 < nlist) issue_stage(std::integral_constant<int, par ^ 1>{}, snext);  // lands before the barrier below
        STAMP(ts1);
        STAMP_ADD(0, ts0, ts1);
        auto mfma_pair = [&](auto p_c) __attribute__((always_inline)) {  // tiles 2 p, 2 p + 1 of the stage
            constexpr int OFF0 = par * STAGE_BYTES + 2 * decltype(p_c)::value * UNIT_BYTES, OFF1 = OFF0 + UNIT_BYTES;
            // the dense kernel's software pipeline over NL k-steps: the fragments of step s + 1 are requested before the
            // MFMAs of step s issue, and a step waits only for ITS two reads (counted lgkmcnt)
            f16x8 fa0[2], fa1[2];
            lds_read128(fa0[0], fa, std::integral_constant<int, OFF0>{});
            lds_read128(fa1[0], fa, std::integral_constant<int, OFF1>{});
            static_for(std::make_integer_sequence<int, NL>{}, [&](auto s_c) {
                constexpr int s = decltype(s_c)::value;
                if constexpr (s < NL - 1) {
                    lds_read128(fa0[(s + 1) & 1], fa, std::integral_constant<int, OFF0 + (s + 1) * 1024>{});
                    lds_read128(fa1[(s + 1) & 1], fa, std::integral_constant<int, OFF1 + (s + 1) * 1024>{});
                    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(fa0[s & 1]), "+v"(fa1[s & 1]));
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa0[s & 1]), "+v"(fa1[s & 1]));
                }
                __builtin_amdgcn_sched_barrier(0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0[s & 1], b[s], s == 0 ? f32x16{} : acc, 0, 0, 0);
                accB = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1[s & 1], b[s], s == 0 ? f32x16{} : accB, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            });
        };
        auto score_pair = [&](const int ts) __attribute__((always_inline)) {
            score(acc, ts);
            if (ts + 1 < nunits) score(accB, ts + 1);  // (the second tile of a last, odd pair is padding)
        };
        if (late && it > 0 && U * sprev + U - 2 < nunits) score_pair(U * sprev + U - 2);
        if (it < nlist) {
            static_for(std::make_integer_sequence<int, NP>{}, [&](auto p_c) {
                constexpr int p = decltype(p_c)::value;
                const int tp = U * scur + 2 * p;
                if (tp < nunits) {  // (wave-uniform; a segment's last stage may hold one pair only)
                    mfma_pair(p_c);
                    if (!late || p < NP - 1) score_pair(tp);
                }
            });
        }
        STAMP(ts2);
        STAMP_ADD(1, ts1, ts2);
        if ((it & FDR_SHARE_EVERY) == FDR_SHARE_EVERY) {
            flush(L, q0, q1);
            share(L, flim);
            cthr = rethreshold(L, flim);
        }
        STAMP(ts3);
        STAMP_ADD(2, ts2, ts3);
#ifdef FDR_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        STAMP(ts3b);
        STAMP_ADD(3, ts3, ts3b);
        __syncthreads();
        STAMP(ts4);
        STAMP_ADD(4, ts3b, ts4);
        if (stamp_on) stamp_acc[5] += 1;
#else
        __syncthreads();  // position it+1 is complete (all waves' pieces) before anyone reads it
#endif
        sprev = scur;
        scur = snext;
        snext = safter;
    };
    const int niter = nlist + 1;  // (one MFMA-less iteration: the late half scores the last stage's last pair)
    for (int it0 = 0; it0 < niter; it0 += 2) {
        stage_body(std::integral_constant<int, 0>{}, it0);
        if (it0 + 1 < niter) stage_body(std::integral_constant<int, 1>{}, it0 + 1);
    }
#ifdef FDR_STAMPS
    if (stamp_on && lane == 0)
        for (int ph = 0; ph < 6; ++ph) atomicAdd(&g_stamps[wave][ph], (unsigned long long)stamp_acc[ph]);
#endif
    const unsigned imask = (1u << ib) - 1u;
    flush(L, q0, q1);
    size_t qrow = (size_t)qb * QW + ql0;
    if (qrow >= (size_t)nq) return;
    qrow = (size_t)ord.perm_q[qrow];  // (always an ordered scan: the lists go back to the rows' own numbers)
    u64 *out = partial + ((size_t)seg * nq_pad + qrow) * K + (h ? (K + 1) >> 1 : 0);
#pragma unroll
    for (int e = 0; e < LH; ++e) {
        if (e >= dead) {
            const unsigned kv = L.v[e];
            u64 o = KEY_INF;
            if (kv != PK_EMPTY) {
                const int trow = ord.perm_t[t_begin + (int)(kv & imask)];
                o = ((u64)__float_as_uint((float)(kv >> ib) / qscale) << 32) | (unsigned)(t_base + trow);
            }
            out[e - dead] = o;
        }
    }
}

typedef void (*LiveKernel)(const _Float16 *, int, const _Float16 *, int, int, SegBounds, int, int, u64 *, unsigned *, int,
                           int, int, const int *, const unsigned *, OrderArgs, const unsigned *, const unsigned *,
                           const int *);
static constexpr LiveKernel kLiveKernels[FDR_LIVE_MAX_NL - FDR_LIVE_MIN_NL + 1] = {
    knn_prefilter_live_kernel<2>, knn_prefilter_live_kernel<3>, knn_prefilter_live_kernel<4>,
    knn_prefilter_live_kernel<5>, knn_prefilter_live_kernel<6>};
static size_t live_lds_bytes(int nl) { return (size_t)2 * 4 * nl * 1024; }  // the ring: two stages of four tiles' live pieces
