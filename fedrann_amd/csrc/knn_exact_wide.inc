// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit), not compiled on its own.
// ------------------------------------------------------------------------------------------
// K3s  tiled exact cosine k-NN for 512 < d <= 1024: K3 (knn_exact.inc) with the components split over two waves.
//
// K3 keeps a wave's 32 queries as the B operand of v_mfma_f32_32x32x2_f32 in DP/2 VGPRs: 512 at DP = 1024, more
// than a wave has.  Here the two waves of a pair share one 32-query set: wave A (part 0) holds components 0..DP/2-1,
// wave B (part 1) the rest, 256 registers each (X512's budget: one wave per SIMD).  A ring stage holds two 64-component
// chunks: chunk c of tile t for A and chunk NCH/2 + c of tile t - 1 for B, so the two waves multiply side by side one
// tile apart.  After its last chunk of a tile A leaves its 16 accumulators per lane in LDS; B starts that tile's chain
// from them.  The sum is therefore K3's fma chain in ascending component order, bit for bit (the same MFMA, the same
// lane layout, the same order of K-steps).  B alone keeps the top-k lists and runs K3's fast path, queues, flushes and
// cross-segment bound on the finished similarities.
// LDS: 2-stage ring of 2 x 8 KB | hand-off 4 KB per pair | lists K x QW keys | queues (QCAP x NT).
// ------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(256, 1) void knn_tile_split_kernel(
    const float *__restrict__ Qh, const unsigned char *__restrict__ qzero, int nq,
    const float *__restrict__ Th, const unsigned *__restrict__ tzbits, int nt, int t_base,
    SegBounds segs, int K, int nq_pad, u64 *__restrict__ partial, unsigned *__restrict__ tau_shared,
    int qcap, int item_base, int nqb FDR_DBG_PARAM) {
#ifndef FDR_DEV
    constexpr int dbg = 0;
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int item = item_base + (int)blockIdx.x;
    const int seg = item / nqb, qb = item - seg * nqb;
    constexpr int NW = 4, NT = 64 * NW;       // waves / threads per workgroup
    constexpr int QW = 32 * NW / 2;           // queries per workgroup: one 32-query set per pair of waves
    constexpr int HC = DP / 128;              // 64-component chunks per part of a tile
    constexpr int CHUNK_BYTES = 32 * 64 * 4;  // 32 target rows x 64 components (8 KB)
    constexpr int STAGE_BYTES = 2 * CHUNK_BYTES;
    constexpr int SLOTS = 16;
    float *handoff = reinterpret_cast<float *>(smem + 2 * STAGE_BYTES);                              // [pair][16][64]
    u64 *lists = reinterpret_cast<u64 *>(smem + 2 * STAGE_BYTES + (NW / 2) * 4096);                  // K * QW keys
    u64 *queues = reinterpret_cast<u64 *>(smem + 2 * STAGE_BYTES + (NW / 2) * 4096 + (size_t)K * QW * 8);  // QCAP * NT

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (uniform: part, t, tile rows in SGPRs)
    const int j = lane & 31, h = lane >> 5;
    const int pair = wave & 1, part = wave >> 1;  // waves 0, 1: part A of pairs 0, 1; waves 2, 3: part B
    float *hand = handoff + pair * 16 * 64;

    // this wave's part of its 32 queries' B fragments: K-steps part * DP/4 .. (part + 1) * DP/4 - 1
    float b[DP / 4];
    const int ql = pair * 32 + j;
    const int qg = qb * QW + ql;
    const int qrow = qg < nq ? qg : nq - 1;
    const bool qz = qzero[qrow] != 0;
    const bool any_qz = __any(qz);
    {
        const f32x4 *qp = reinterpret_cast<const f32x4 *>(Qh + (size_t)qrow * DP) + part * (DP / 8);
#pragma unroll
        for (int g = 0; g < DP / 16; ++g) {
            const f32x4 v = qp[2 * g + h];
            b[4 * g + 0] = v.x;
            b[4 * g + 1] = v.y;
            b[4 * g + 2] = v.z;
            b[4 * g + 3] = v.w;
        }
    }
    for (int i = tid; i < K * QW; i += NT) lists[i] = KEY_INF;
    TopkState st;
    st.taukey = KEY_INF;
    st.taupos = 0;
    st.qcnt = 0;
    st.tau = topk_share(tau_shared + qg, KEY_INF, h, st.foreign);
    st.cfloor = sim_floor(st.tau);

    const int t_begin = segs.b[seg];
    const int t_end = min(nt, segs.b[seg + 1]);
    const int ntiles = (t_end - t_begin + 31) >> 5;
    const int nsteps = (ntiles + 1) * HC;  // step i: A on chunk i % HC of tile i / HC, B on chunk HC + i % HC of tile i / HC - 1

    // a stage's 16 pieces of 1 KiB (four staged rows each, K3's source-side XOR swizzle): pieces 0..7 A's chunk,
    // 8..15 B's; four per wave
    auto issue_stage = [&](int i, int buf) {
        const int tt = i / HC, c = i % HC;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int piece = wave + NW * u, pp = piece & 7, pt = piece >> 3;
            const int t = tt - pt;  // (part B stages the previous tile)
            if (t < 0 || t >= ntiles) continue;
            const int ch = pt * HC + c;
            const int row = 4 * pp + (lane >> 4), pslot = lane & 15;
            const int trow = min(t_begin + t * 32 + row, t_end - 1);
            const float *src = Th + (size_t)trow * DP + (size_t)(ch * SLOTS + (pslot ^ (row & 15))) * 4;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)src,
                (__attribute__((address_space(3))) void *)(smem + buf * STAGE_BYTES + piece * 1024), 16, 0, 0);
        }
    };

    if (ntiles > 0) issue_stage(0, 0);
    __syncthreads();  // also publishes the list initialisation

    for (int tt = 0; tt <= ntiles && ntiles > 0; ++tt) {
        const int t = tt - part;               // the tile this wave works on in this round of steps
        const bool active = t >= 0 && t < ntiles;  // (wave-uniform)
        f32x16 acc;
#pragma unroll
        for (int c = 0; c < HC; ++c) {
            const int i = tt * HC + c;
            const int buf = i & 1;
            if (i + 1 < nsteps) issue_stage(i + 1, (i + 1) & 1);
            if (active) {
                if (c == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = part == 0 ? 0.f : hand[r * 64 + lane];
                }
                const f32x4 *sb = reinterpret_cast<const f32x4 *>(smem + buf * STAGE_BYTES + part * CHUNK_BYTES) + j * SLOTS;
                const int sw = j & 15;
                f32x4 a[3];
                a[0] = sb[(0 + h) ^ sw];
                a[1] = sb[(2 + h) ^ sw];
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    if (g + 2 < 8) a[(g + 2) % 3] = sb[(2 * (g + 2) + h) ^ sw];
                    const f32x4 av = a[g % 3];
                    const int bb = 32 * c + 4 * g;
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b[bb + e], acc, 0, 0, 0);
                }
                if (c == HC - 1 && part == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) hand[r * 64 + lane] = acc[r];  // (B reads it after the barrier below)
                }
                if (c == HC - 1 && part == 1) {
                    const int tile_row0 = t_begin + t * 32;
                    if (any_qz) {  // an all-zero query is at distance 0 from all-zero targets, 1 from the rest
                        const unsigned zm = tzbits[(t_begin >> 5) + t] >> (4 * h);
                        if (qz) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[r] = (float)((zm >> ((r & 3) + 8 * (r >> 2))) & 1u);
                        }
                    }
                    float mx = acc[0];
#pragma unroll
                    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[r]);
                    if (__any(mx > st.cfloor))
                        topk_append<NT, QW>(acc, st, lists, queues, tau_shared + qg, ql, K, tid, h, t_base + tile_row0,
                                            t_end - tile_row0, qcap, (dbg & 2) != 0);
                    if ((t & 31) == 31 && !(dbg & 4)) {
                        st.tau = topk_share(tau_shared + qg, st.taukey, h, st.foreign);
                        st.cfloor = sim_floor(st.tau);
                    }
                }
            }
            __syncthreads();  // stage i + 1 has landed; A's hand-off is visible to B
        }
    }

    if (part == 1 && __any(st.qcnt > 0))
        st = topk_flush<NT, QW>(st, lists, queues, tau_shared + qg, ql, K, tid, h, qcap, (dbg & 2) != 0);
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
