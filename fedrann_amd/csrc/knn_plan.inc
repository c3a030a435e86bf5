// Part of libfedrann_hip.so (included by fedrann_hip.hip) and of the host-only sanitizer build
// (tests/host_san/host_san.cpp): the k-NN launch planner -- kernel shapes, LDS budgets, the split of the
// targets into segments.  Plain C++, no HIP.
#define QCAP 4  // default entries per lane append queue (the kernels take the actual value, 2 or 4)
#define FDR_MAX_SEG 96
// what the MFMA kernels cover (FDR_MAX_K / FDR_MAX_DIM of the header are the generic kernel's limits, knn_generic.inc):
// every pass (fp16 prefilter, exact, duplicate-row classes) up to FDR_FAST_MAX_K / _DIM; the exact pass alone up to
// FDR_EXACT_MAX_K neighbours from FDR_WIDE_MIN_TARGETS targets (knn_route)
#define FDR_FAST_MAX_K 64
#define FDR_FAST_MAX_DIM 512
#define FDR_EXACT_MAX_K 128
#define FDR_EXACT_MAX_DIM 1024   // (d > 512: the split-K tile kernel, knn_exact_wide.inc)
#define FDR_MERGE_WIDE_CAP 1024  // keys per query the k > 64 merge stages in LDS (knn_merge_wide_kernel)
#define FDR_WIDE_MIN_TARGETS 8192  // (AUTO's prefilter threshold; a function of nt alone: every rank decides alike)

// Target segment boundaries (in rows, multiples of 32 except the last): segment s = [b[s], b[s+1]).
struct SegBounds {
    int b[FDR_MAX_SEG + 1];
};


static int padded_dim(int d) {  // row length (floats) of the normalised-embedding layout
    if (d <= 0) return FDR_E_ARG;
    if (d <= 128) return 128;
    if (d <= 256) return 256;
    if (d <= 512) return 512;
    if (d <= 1024) return 1024;  // (the split-K tile kernel, knn_exact_wide.inc; below 8192 targets the generic kernel)
    if (d <= FDR_MAX_DIM) return 2048;
    return FDR_E_ARG;
}

// (bounds |fp16 pass distance - canonical distance| with the grid term of prefilter_eps(); the device's own candidate
// lists are checked against it on adversarial rows in tests/test_gpu_candidates.py, test_candidates_on_adversarial_rows)
#define FDR_PREFILTER_EPS 0.00105f
#define FDR_PREFILTER_EXTRA 8

// Key layout of the prefilter pass (see RegList): ib index bits for the longest segment, the rest (at
// most 20) for the quantised distance.  At least 13 distance bits, i.e. segments of at most 2^19 rows.
#define FDR_PREFILTER_MAX_IB 19
static int prefilter_index_bits(int max_segment_rows) {
    int ib = 8;
    while ((1ll << ib) < max_segment_rows) ++ib;
    return ib;
}
// |approximate distance - canonical distance| of a prefilter candidate: fp16 operands + the key grid
static float prefilter_eps(int ib) {
    const int qbits = std::min(20, 32 - ib);
    return FDR_PREFILTER_EPS + 0.5f / (float)((1u << qbits) - 2u) + 1.0e-6f;
}

// The threshold margin of the dense index's radius search (knn_dense_radius.inc): its fp16 range pass admits
// d~ <= th, th = r + radius_margin(), and the canonical chain then decides dist <= r.  No key-grid term: nothing is
// quantised there.  Proof that {d~ <= th} holds every hit: dist <= r and |d~ - dist| <= FDR_PREFILTER_EPS give
// d~ <= r + FDR_PREFILTER_EPS; the fp32 rounding of the sum r + M (r < 1, so the sum is below 2) is below 1.2e-7,
// which the 1.0e-6 covers.  th >= 1 is legal: every row is a candidate then, and max_hits decides.
static float radius_margin() { return FDR_PREFILTER_EPS + 1.0e-6f; }

// The target chunks of that search.  A plan of the fp16 shapes holds at most FDR_MAX_SEG segments of at most
// 2^FDR_PREFILTER_MAX_IB rows (knn_plan_compute; the k-NN search leaves the prefilter mode above that many targets,
// knn_prefilter_wanted), so an index of more rows is scanned in chunks of at most that many, each with a plan of its
// own and its first row as t_base: equal chunks, a multiple of 32 rows each but the last.
#define FDR_RADIUS_CHUNK_ROWS ((int64_t)FDR_MAX_SEG << FDR_PREFILTER_MAX_IB)
static int64_t radius_chunks(int64_t n) { return n <= 0 ? 0 : (n + FDR_RADIUS_CHUNK_ROWS - 1) / FDR_RADIUS_CHUNK_ROWS; }
static int64_t radius_chunk_rows(int64_t n) {  // rows of every chunk but the last
    const int64_t c = radius_chunks(n);
    return c == 0 ? 0 : ((n + c - 1) / c + 31) / 32 * 32;
}

// Candidates kept beyond k.  k + 8 is the base; k + 12 when that costs no registers (the two lanes of a query hold
// 2 x 16 or 2 x 32 keys: K' = 32 for k = 20, K' = 62 for k = 50) -- at 10 M rows (config 4) the queries that cannot be
// certified from K' candidates and go through the range pass fall from 165 k to 99 k of 916 k (a rank's k-NN: 0.713 ->
// 0.661 s); at 1 M rows 9341 -> 1124, the pass 1.2 ms longer, the range pass 1.3 ms shorter.  K' = 36 for k = 20 (2 x 32
// keys) loses more in the pass than the range pass gains.  (development knob FDR_KNN_EXTRA)
static int prefilter_extra(int k) {
    const int forced = dev_knobs().extra;
    if (forced >= 2 && forced <= 44) return forced;
    const int width = k + FDR_PREFILTER_EXTRA <= 32 ? 32 : 64;  // keys the register lists hold at k + 8
    return k + 12 <= width ? 12 : FDR_PREFILTER_EXTRA;
}

// Kernel shapes: one entry per kernel a pass can launch (the candidate pass: per list width), so that an index names
// the kernel.  queries/workgroup QW = 32*NQ*NW; slots = workgroups resident per CU (LDS- and register-limited).  The
// passes choose among them with knn_choose_shape() (exact), prefilter_shape() (candidates) and range_shape() (range).
enum KnnFamily {
    FDR_FAM_TILE,       // knn_tile_kernel<DP, NQ, NW, WPS> (knn_exact.inc): the exact fp32 pass
    FDR_FAM_PREFILTER,  // knn_prefilter_kernel<DP, NQ, NW, WPS, U, LH, PAIRED> (knn_prefilter.inc): fp16 candidates
    FDR_FAM_PINGPONG,   // knn_prefilter_pp_kernel<DP, U, LH> (knn_prefilter_pp.inc): eight waves, 256 registers
    FDR_FAM_RANGE,      // knn_range_kernel<DP, NW, WPS> (knn_prefilter.inc): the range pass over plateau queries
    FDR_FAM_RANGE_PP,   // knn_range_pp_kernel<DP, U> (knn_prefilter_pp.inc): the range pass, ping-pong skeleton
    FDR_FAM_TILE_SPLIT, // knn_tile_split_kernel<DP> (knn_exact_wide.inc): the exact fp32 pass, K split over two waves
};
struct KnnShape {
    int family, dp, nq, nw, wps;
    int tps;       // fp16 passes: the LDS ring's one-tile (8 KB) units, two stages of units() each; 0: the fp32 tile kernel
    bool paired;   // candidate pass, 16-key lists: the stage's two tiles as two interleaved MFMA chains (d <= 128: 1-4 %)
    int lists;     // candidate pass: the list widths (16 / 32 keys a lane, K' <= 32 / > 32) it is compiled for, or'ed
    bool release;  // chosen with the default knobs: compiled into the release library (a development build: every entry)
    int split = 1; // waves that share one 32-query set, each holding a part of its components (FDR_FAM_TILE_SPLIT: 2)
    constexpr int units() const { return tps / 2; }  // the stage's units U
    constexpr int qw() const { return 32 * nq * nw / split; }  // queries per workgroup
};
enum KnnShapeId {
    FDR_X128, FDR_X128_W8, FDR_X128_Q2, FDR_X256, FDR_X512,
    FDR_P128, FDR_P128_W8, FDR_P128_W8U4, FDR_P256, FDR_P256_V2, FDR_P256_W8, FDR_P256_U4, FDR_P256_W8U4, FDR_P256_W8U8,
    FDR_P512, FDR_P512_U4, FDR_P512_W8U4,
    FDR_PP256, FDR_PP512_U8, FDR_PP512_U4,
    FDR_R128, FDR_R128_W8, FDR_R256, FDR_R512, FDR_RPP128, FDR_RPP256, FDR_RPP512,
    FDR_X256_W4, FDR_X1024,
    FDR_NUM_SHAPES
};
static constexpr KnnShape kShapes[] = {
    // the exact tile kernel
    {FDR_FAM_TILE, 128, 1, 4, 3, 0, false, 0, true},   // X128: 128 queries/WG, <=168 VGPRs, up to 3 WG/CU
    {FDR_FAM_TILE, 128, 1, 8, 4, 0, false, 0, false},  // X128_W8: 256 queries/WG, <=128 VGPRs, up to 2 WG/CU (knob SHAPE)
    {FDR_FAM_TILE, 128, 2, 4, 2, 0, false, 0, true},   // X128_Q2: 256 queries/WG, <=256 VGPRs, up to 2 WG/CU
    {FDR_FAM_TILE, 256, 1, 8, 2, 0, false, 0, true},   // X256: 256 queries/WG, <=256 VGPRs, 1 WG/CU
    {FDR_FAM_TILE, 512, 1, 4, 1, 0, false, 0, true},   // X512: 128 queries/WG, one wave per SIMD: 512 registers per lane
                                                       // (256 of them queries)
    // fp16 candidate pass (LDS = the ring only): 128 queries/WG, two-unit stages (32 KB ring).  One-unit stages (a barrier
    // per 8 MFMAs) cost +25 % at d <= 128, three / four-unit stages lose workgroups per CU, two query sets per wave
    // (NQ = 2, 192 VGPRs) lost 10-25 % to the lower occupancy.
    {FDR_FAM_PREFILTER, 128, 1, 4, 4, 4, true, 48, true},  // P128: d <= 128, <= 128 VGPRs, 4 WG/CU
    // eight waves per workgroup (256 queries, 2 WG/CU): every staged tile serves twice the queries, half the L2 -> LDS
    // traffic and LDS-DMA instructions per flop (devtools/mfma_shape_bench.hip: 0.67 -> 0.76 of the peak for the bare loop);
    // W8U4: FOUR-unit stages (two pairs of tiles per barrier, 64 KB ring, 2 WG/CU)
    {FDR_FAM_PREFILTER, 128, 1, 8, 4, 4, true, 16, false},  // P128_W8 (knob W8 = 2)
    {FDR_FAM_PREFILTER, 128, 1, 8, 4, 8, true, 16, true},   // P128_W8U4
    {FDR_FAM_PREFILTER, 256, 1, 4, 3, 4, false, 48, true},  // P256: d <= 256, <= 168 VGPRs, one tile per stage
    // d <= 256 at 256 VGPRs: all eight fragments of a unit in flight (the d <= 512 kernel's inner loop), two workgroups per
    // CU on two queues; and the same with eight waves (256 queries, one workgroup per CU)  (knob D256 = 1 / 2)
    {FDR_FAM_PREFILTER, 256, 1, 4, 2, 4, false, 48, false},  // P256_V2
    {FDR_FAM_PREFILTER, 256, 1, 8, 2, 4, false, 48, false},  // P256_W8
    // the 256-VGPR shapes with four-unit stages: a 64 KB ring, still two workgroups per CU (d <= 256 with K' > 32, d <= 512)
    {FDR_FAM_PREFILTER, 256, 1, 4, 2, 8, false, 32, true},  // P256_U4
    // the same with eight waves -- 256 queries per staged tile, one workgroup per CU (d <= 256 with K' > 32; knob D256 = 4),
    // and with eight-unit stages, a 128 KB ring (D256 = 5, or the ping-pong sizes with PP = 0)
    {FDR_FAM_PREFILTER, 256, 1, 8, 2, 8, false, 32, false},   // P256_W8U4
    {FDR_FAM_PREFILTER, 256, 1, 8, 2, 16, false, 32, false},  // P256_W8U8
    {FDR_FAM_PREFILTER, 512, 1, 4, 2, 4, false, 48, false},   // P512: d <= 512, 128 VGPRs of queries, half a tile per stage
    {FDR_FAM_PREFILTER, 512, 1, 4, 2, 8, false, 48, true},    // P512_U4
    {FDR_FAM_PREFILTER, 512, 1, 8, 2, 8, false, 48, false},   // P512_W8U4: development only, measured slower (D256 = 4)
    // The ping-pong kernel (eight waves, 256 registers, one workgroup per CU): d <= 256 with eight-unit stages; d <= 512
    // with eight-unit stages for K' <= 32 and four-unit ones for K' > 32 (128 query + 33 list registers leave room for one
    // tile's accumulators).  (d <= 128 measured 0.745 against 0.90 without the cold path and was dropped.)
    {FDR_FAM_PINGPONG, 256, 1, 8, 2, 16, false, 48, true},  // PP256
    {FDR_FAM_PINGPONG, 512, 1, 8, 2, 16, false, 16, true},  // PP512_U8
    {FDR_FAM_PINGPONG, 512, 1, 8, 2, 8, false, 32, true},   // PP512_U4
    // the range pass: the candidate pass's geometry, RANGE_STAGES one-unit stages (d > 128: compiled for 256 VGPRs; at
    // d <= 256 it takes 148, so the three workgroups per CU of wps = 3 fit); from 4096 plateau queries the ping-pong
    // skeleton with eight-unit stages.  The radius search of the dense index (knn_dense_radius.inc) runs the same
    // entries with its counting and emitting sinks over ALL queries of a call x the plan's segments: R128 / R256 / R512
    // below 4096 queries, RPP128 / RPP256 / RPP512 from there (range_shape(dp, nq, nq))
    {FDR_FAM_RANGE, 128, 1, 4, 4, 4, false, 0, true},      // R128
    {FDR_FAM_RANGE, 128, 1, 8, 4, 4, false, 0, true},      // R128_W8
    {FDR_FAM_RANGE, 256, 1, 4, 3, 4, false, 0, true},      // R256
    {FDR_FAM_RANGE, 512, 1, 4, 2, 4, false, 0, true},      // R512
    {FDR_FAM_RANGE_PP, 128, 1, 8, 2, 16, false, 0, true},  // RPP128
    {FDR_FAM_RANGE_PP, 256, 1, 8, 2, 16, false, 0, true},  // RPP256
    {FDR_FAM_RANGE_PP, 512, 1, 8, 2, 16, false, 0, true},  // RPP512
    // the exact tile kernel for 64 < k <= 128 (knn_choose_shape): lists of k x 128 queries x 8 bytes (up to 128 KiB)
    // leave room for one workgroup per CU, so 128 queries per workgroup, one wave per SIMD; d <= 128 and d <= 512
    // take X128 and X512, d <= 256 this one (X256's 256 queries would not fit above k = 70)
    {FDR_FAM_TILE, 256, 1, 4, 2, 0, false, 0, true},  // X256_W4: 128 queries/WG, <=256 VGPRs
    // d <= 1024 (k <= 128): a wave holds 512 of a query's components (256 registers, X512's budget), so two waves -- one
    // per SIMD -- share a 32-query set: 64 queries/WG, one WG/CU
    {FDR_FAM_TILE_SPLIT, 1024, 1, 4, 1, 0, false, 0, true, 2},  // X1024
};
static_assert(sizeof(kShapes) / sizeof(kShapes[0]) == FDR_NUM_SHAPES, "one kShapes entry per KnnShapeId");

static int prefilter_shape(int dp, int kp, int64_t nq, int num_cus, int64_t nt = 0) {  // kp = K' = candidates per query of the pass
    // d <= 128: eight waves per workgroup once the 256-query blocks fill (nearly) a round of two workgroups per CU --
    // 100.1 -> 97.7 ms at 1 M rows, 15.1 -> 14.6 ms for a rank's eighth of them; 100 k rows (391 blocks): 2.7 -> 3.0 ms,
    // so smaller sets keep four waves.
    // Four-unit stages (round 4: two pairs of tiles per barrier, a 64 KB ring, still two workgroups per CU): 95.4 -> 94.2 ms
    // at 1 M rows, 747 -> 742 at 4 M, and no spill at 128 registers (the two-unit form: 20 bytes).
    // (development knob W8: 0 never the eight-wave shape, 3 always, 2 the two-unit stages of round 3)
    const int w8 = dev_knobs().w8;
    // A rank's slice (a few hundred query blocks against several times as many target rows: long segments) takes the
    // eight-wave shape from one block per CU -- 1 M / 8: the pass 13.8 -> 13.6 ms on its share of the unique rows, 15.0 -> 13.5 on
    // its row block; all-pairs sets of that size (100 k rows: 391 blocks) keep four waves (2.55 against 2.81 ms).
    const int64_t blocks = (nq + 255) / 256;
    const bool fills = blocks * 10 >= (int64_t)num_cus * 2 * 9 || (blocks >= num_cus && nt >= 4 * nq);
    if (dp == 128 && kp <= 32 && (w8 == 3 || ((w8 == 1 || w8 == 2) && fills)))
        return w8 == 2 ? FDR_P128_W8 : FDR_P128_W8U4;
    // d > 128: the ping-pong kernel once its 256-query blocks fill two launches of one workgroup per CU (round 4; same box,
    // round 3's shapes -> ping-pong): d = 256 / k = 50 at 1 M doubled rows 330 -> 323 ms, at 4 M 4.00 -> 3.40 s (0.67 -> 0.79 of
    // the fp16 peak), a rank of config 5 10.9 -> 8.8 s (0.68 -> 0.84); d = 256 / k = 20 at 1 M doubled rows 324 -> 290 ms;
    // d = 500 / k = 50 at 600 k rows 251 -> 221 ms, k = 20 246 -> 203 ms.  Its phases wait for the slowest of four scoring
    // waves, so it gains the more the rarer insertions are: smaller sets keep round 3's four-wave shapes below.
    // (development knob PP: 0 = never, 1 = at every size)
    const int pp = dev_knobs().pp;
    const bool pp_fills = (nq + 255) / 256 >= (int64_t)num_cus * 2;
    if (dp == 256 && (pp == 1 || (pp < 0 && pp_fills))) return FDR_PP256;
    if (dp == 512 && (pp == 1 || (pp < 0 && pp_fills))) return kp <= 32 ? FDR_PP512_U8 : FDR_PP512_U4;
    // Round 3's shapes.  d <= 256 with K' > 32 (the 2 x 32-key register lists): 64 fragment + 33 list + 16 accumulator
    // registers do not fit the 168-VGPR shape without spills -- at 256 VGPRs, two workgroups per CU on two queues, all
    // eight fragments of a unit in flight and four-unit stages: 575 -> 372 ms at 1 M doubled rows, k = 50 (K' <= 32 keeps the
    // three-per-CU shape: 327 against 358 ms at k = 20).  d <= 512 was at 256 VGPRs already; four-unit stages: 272 -> 264 ms.
    // (knob D256: 1 / 2 = two-unit stages / eight waves and one workgroup per CU, 4 / 5 = the eight-wave shape with four- /
    // eight-unit stages: development, with PP = 0)
    const int v256 = dev_knobs().d256;
    if (dp == 256 && v256 == 1) return FDR_P256_V2;
    if (dp == 256 && v256 == 2) return FDR_P256_W8;
    if (dp == 256 && kp > 32 && v256 == 4) return FDR_P256_W8U4;
    if (dp == 256 && kp > 32 && (v256 == 5 || (v256 == 3 && pp == 0 && pp_fills))) return FDR_P256_W8U8;
    if (dp == 256 && v256 == 3 && kp > 32) return FDR_P256_U4;
    if (dp == 512 && v256 == 4) return FDR_P512_W8U4;
    if (dp == 512 && v256 == 3) return FDR_P512_U4;
    return dp == 128 ? FDR_P128 : dp == 256 ? FDR_P256 : FDR_P512;
}

// The range pass over `chunk` of its `plateau` queries.  From 4096 queries (16 blocks of 256, times the plan's segments)
// it runs on the ping-pong skeleton (eight waves, one workgroup per CU, eight-unit stages); a handful of them (1 M rows:
// 1100) keeps round 3's kernel with its many short segments.  (d <= 128, many plateau queries: round 3's eight-wave form,
// development knob RANGE8 with RANGEPP = 0)
static int range_shape(int dp, int chunk = 0, int plateau = 0) {  // (dp alone: the four-wave kernel of a few queries)
    const int r8 = dev_knobs().range8, rpp = dev_knobs().rangepp;
    if (rpp == 1 || (rpp < 0 && chunk >= 4096)) return dp == 128 ? FDR_RPP128 : dp == 256 ? FDR_RPP256 : FDR_RPP512;
    if (dp == 128 && (r8 == 1 || (r8 < 0 && plateau >= 65536))) return FDR_R128_W8;
    return dp == 128 ? FDR_R128 : dp == 256 ? FDR_R256 : FDR_R512;
}

static size_t knn_lds_bytes_q(const KnnShape &sh, int k, int qcap) {
    const size_t qw = (size_t)sh.qw(), nt = (size_t)64 * sh.nw;
    if (sh.tps > 0) return (size_t)sh.tps * 32 * 256;  // fp16 prefilter: the ring only (lists in registers)
    // split K: a ring stage holds one 64-component chunk per part, and each pair hands 32 x 32 partial sums over
    const size_t ring = (size_t)2 * 32 * 64 * 4 * sh.split, handoff = sh.split > 1 ? (size_t)(sh.nw / sh.split) * 4096 : 0;
    return ring + handoff + (size_t)k * qw * 8 + (size_t)qcap * sh.nq * nt * 8;
}

// Entries per lane append queue: 4, or 2 when that lets one more workgroup share the CU's LDS
// (co-resident workgroups matter more than the flush rate).
static int knn_qcap(const KnnShape &sh, int k) {
    const size_t lds = 160 * 1024;
    const int with4 = (int)(lds / knn_lds_bytes_q(sh, k, 4)), with2 = (int)(lds / knn_lds_bytes_q(sh, k, 2));
    const int by_regs = std::max(1, (sh.wps * 4) / sh.nw);
    return std::min(with2, by_regs) > std::min(with4, by_regs) ? 2 : QCAP;
}

static size_t knn_lds_bytes(const KnnShape &sh, int k) { return knn_lds_bytes_q(sh, k, knn_qcap(sh, k)); }

static int knn_wg_per_cu(const KnnShape &sh, int k) {
    const int by_lds = (int)((size_t)160 * 1024 / knn_lds_bytes(sh, k));
    const int by_regs = (sh.wps * 4) / sh.nw;  // waves per CU the register budget allows / waves per WG
    return std::max(0, std::min(by_lds, std::max(by_regs, 1)));
}

static int knn_choose_shape(int dp, int k) {
    const int forced = dev_knobs().shape;
    if (forced >= 0 && forced < FDR_NUM_SHAPES && kShapes[forced].family == FDR_FAM_TILE && kShapes[forced].dp == dp &&
        knn_wg_per_cu(kShapes[forced], k) > 0)
        return forced;
    if (dp == 1024) return FDR_X1024;
    if (k > FDR_FAST_MAX_K) return dp == 128 ? FDR_X128 : dp == 256 ? FDR_X256_W4 : FDR_X512;  // (128 queries/WG)
    if (dp == 256) return FDR_X256;
    if (dp == 512) return FDR_X512;
    // d <= 128: the 4-wave / 128-query shape (no spills at 168 VGPRs, finest work granularity) while
    // at least two workgroups fit in LDS; for larger k the 2-chain 256-VGPR shape
    if (knn_wg_per_cu(kShapes[FDR_X128], k) >= 2) return FDR_X128;
    return FDR_X128_Q2;
}

// Which kernels a k-NN call of padded dimension dp, k neighbours and nt targets runs on.  Every entry point (the
// workspace size, the class layer, the search) takes its decision from here.
enum KnnRoute {
    FDR_ROUTE_FAST,     // k <= 64, d <= 512: exact or fp16-prefilter MFMA passes, duplicate-row classes
    FDR_ROUTE_WIDE,     // 64 < k <= 128 at d <= 512, or k <= 128 at 512 < d <= 1024, nt >= 8192: the exact MFMA pass
                        // alone (no prefilter, no classes)
    FDR_ROUTE_GENERIC,  // the rest: knn_generic_kernel (knn_generic.inc)
};
static int knn_route(int dp, int k, int64_t nt) {
    if (dp <= FDR_FAST_MAX_DIM && k <= FDR_FAST_MAX_K) return FDR_ROUTE_FAST;
    if (dp <= FDR_EXACT_MAX_DIM && k <= FDR_EXACT_MAX_K && nt >= FDR_WIDE_MIN_TARGETS) return FDR_ROUTE_WIDE;
    return FDR_ROUTE_GENERIC;
}

struct KnnPlan {
    int shape, qw, nqb, nseg, nq_pad;
    int cohort;  // > 0: launch the nqb * nseg work items in groups of this many workgroups (see knn_plan_compute)
    int queues;  // ... dealt round-robin to this many queues (1: one launch after the other)
    SegBounds segs;
    size_t bits_bytes;     // packed zero-target flags, at the start of the workspace
    size_t shared_bytes;   // one cross-segment bound word per (padded) query
    size_t partial_bytes;  // per-segment top-k lists
    size_t total_bytes;
};

// Makespan (in 32-row tiles) of dispatching, in order, nqb workgroups per segment onto `slots`
// concurrently resident workgroups; every workgroup costs its segment's tiles + `ov` tiles of fixed
// work (query load, list set-up, final flush and write-out).  A workgroup takes the slot that frees
// first.  All workgroups of a segment last equally long, so their finish times leave in the order
// their start times arrive: the slots are kept as runs (free time, count) in two sorted queues -- the
// slots not yet used by this segment and the ones it has already re-filled -- and a whole run is
// dispatched at once.  (One heap operation per workgroup took minutes for the 156 k query blocks of a
// 20 M-row search; this is O(runs * rounds).)
static double simulate_makespan(const std::vector<int> &seg_tiles, int nqb, int slots, double ov) {
    struct Run {
        double t;
        long long n;
    };
    std::vector<Run> old_q{{0.0, (long long)slots}}, new_q, merged;
    double last = 0.0;
    for (int tiles : seg_tiles) {
        const double dur = (double)tiles + ov;
        new_q.clear();
        size_t io = 0, in = 0;  // fronts of the two queues
        long long left = nqb;
        while (left > 0) {
            const bool from_old = io < old_q.size() && (in >= new_q.size() || old_q[io].t <= new_q[in].t);
            Run &src = from_old ? old_q[io] : new_q[in];
            const long long c = std::min(src.n, left);
            const double done = src.t + dur;  // (>= every finish time queued so far: starts are non-decreasing)
            src.n -= c;
            left -= c;
            if (src.n == 0) (from_old ? io : in)++;
            if (!new_q.empty() && new_q.back().t == done) new_q.back().n += c;
            else new_q.push_back(Run{done, c});
            last = std::max(last, done);
        }
        merged.clear();
        while (io < old_q.size() || in < new_q.size()) {
            const bool from_old = io < old_q.size() && (in >= new_q.size() || old_q[io].t <= new_q[in].t);
            const Run r = from_old ? old_q[io++] : new_q[in++];
            if (r.n == 0) continue;
            if (!merged.empty() && merged.back().t == r.t) merged.back().n += r.n;
            else merged.push_back(r);
        }
        old_q.swap(merged);
    }
    return last;
}

static KnnPlan knn_plan_compute(int num_cus, int64_t nq, int64_t nt, int d, int k, int shape);

// Synchronised rounds cut the targets into at most this many segments more than the key layout requires.
#define FDR_COHORT_EXTRA_SEG 7
#define FDR_PLAN_EXTRA_SEG 9  // no fp16-prefilter plan has more segments than this beyond what the key layout requires
// Upper bound of the partial-list bytes of ANY fp16-prefilter plan for nq' <= nq queries and nt' <= nt targets
// (the workspace of a call is sized before the duplicate-row layer knows how many unique rows it will search).
static size_t prefilter_partial_bound(int64_t nq, int64_t nt, int kp, int qw) {
    const int64_t T = (nt + 31) / 32, cap = (1 << FDR_PREFILTER_MAX_IB) / 32;
    const int64_t c0 = (T + cap - 1) / cap;
    const int64_t nseg = std::min<int64_t>(FDR_MAX_SEG, c0 + FDR_PLAN_EXTRA_SEG);
    const int64_t qwm = std::max(qw, 256);  // (the later call may take the other shape: pad for the wider query block)
    const int64_t nq_pad = (nq + qwm - 1) / qwm * qwm;
    return (size_t)nseg * (size_t)nq_pad * (size_t)kp * 8;
}

// the plan search simulates a few hundred dispatch orders: remember the last few results
struct PlanCacheEntry {
    int64_t nq, nt;
    int dp, k, cus, shape;
    KnnPlan plan;
};
static thread_local std::vector<PlanCacheEntry> g_plan_cache;

static KnnPlan knn_plan(int num_cus, int64_t nq, int64_t nt, int d, int k, int shape = -1) {
    const int dp = padded_dim(d);
    for (const PlanCacheEntry &e : g_plan_cache)
        if (e.nq == nq && e.nt == nt && e.dp == dp && e.k == k && e.cus == num_cus && e.shape == shape) return e.plan;
    PlanCacheEntry e{nq, nt, dp, k, num_cus, shape, knn_plan_compute(num_cus, nq, nt, d, k, shape)};
    if (g_plan_cache.size() >= 16) g_plan_cache.erase(g_plan_cache.begin());
    g_plan_cache.push_back(e);
    {
        if (dev_knobs().debug & 8) {
            fprintf(stderr, "[fdr plan] nq=%lld nt=%lld shape=%d nqb=%d nseg=%d cohort=%d tiles:", (long long)nq,
                    (long long)nt, e.plan.shape, e.plan.nqb, e.plan.nseg, e.plan.cohort);
            for (int i = 0; i < e.plan.nseg; ++i)
                fprintf(stderr, " %d", (e.plan.segs.b[i + 1] - e.plan.segs.b[i]) / 32);
            fprintf(stderr, "\n");
        }
    }
    return e.plan;
}

static KnnPlan knn_plan_compute(int num_cus, int64_t nq, int64_t nt, int d, int k, int shape) {
    KnnPlan p;
    p.shape = shape >= 0 ? shape : knn_choose_shape(padded_dim(d), k);
    const KnnShape &sh = kShapes[p.shape];
    p.qw = sh.qw();
    p.nqb = (int)((nq + p.qw - 1) / p.qw);
    p.nq_pad = p.nqb * p.qw;
    // Work split.  The grid is nqb query blocks x nseg target segments; workgroups are dispatched
    // segment by segment onto `slots` resident workgroups.  Equal segments leave the last "round"
    // mostly empty whenever nqb * nseg is not just below a multiple of `slots`, so the plan is a few
    // long segments followed by shorter ones that fill the tail (guided self-scheduling), chosen by
    // simulating the dispatch.  Segments of one query block share their bound (topk_share), so the
    // extra segments cost little more than their fixed set-up (`ov`, in tiles).
    int slots = num_cus * std::max(1, knn_wg_per_cu(sh, k));
    // fp16 prefilter: a fourth workgroup on a CU hides latency but shares the same MFMA / LDS pipes; the
    // dispatch model that matched the measurements best counts three (100 k rows: 3.3 ms vs 3.9 ms)
    if (sh.tps > 0 && sh.nq == 1) slots = std::min(slots, num_cus * 3);
    const DevKnobs K = dev_knobs();
    if (K.slots > 0) slots = num_cus * K.slots;
    const int T = (int)((nt + 31) / 32);  // tiles
    double ov = sh.tps > 0 ? 96.0 : 16.0;  // fp16 tiles are 16x shorter: the fixed cost weighs more
    if (K.ov > 0.0) ov = K.ov;
    // fp16 prefilter keys index rows inside a segment with at most FDR_PREFILTER_MAX_IB bits
    const int cap_tiles = sh.tps > 0 ? (1 << FDR_PREFILTER_MAX_IB) / 32 : T;
    std::vector<int> best;
    {
        const int c0 = (T + cap_tiles - 1) / cap_tiles, l0 = (T + c0 - 1) / c0;
        for (int left = T; left > 0; left -= l0) best.push_back(std::min(left, l0));
    }
    double best_cost = simulate_makespan(best, p.nqb, slots, ov);
    const int min_tiles = sh.tps > 0 ? 128 : 24;  // never cut segments shorter than 768 (4096) rows
    for (int cmain = 1; cmain <= 24; ++cmain)
        for (int tf = 0; tf <= 4; ++tf)          // share of the tiles given to the short tail
            for (int div = 2; div <= 8; div *= 2) {  // tail segments are 1/div of a main segment
                const double tail_frac = 0.08 * tf;
                if (tf == 0 && div != 2) continue;
                const int main_total = (int)((1.0 - tail_frac) * T);
                const int lm = std::max(min_tiles, (main_total + cmain - 1) / cmain);
                std::vector<int> segs;
                int left = T;
                for (int i = 0; i < cmain && left > 0; ++i) {
                    const int t = std::min(left, lm);
                    segs.push_back(t);
                    left -= t;
                }
                const int ls = std::max(min_tiles, lm / div);
                while (left > 0) {
                    const int t = (left < ls + min_tiles) ? left : ls;
                    segs.push_back(t);
                    left -= t;
                }
                if ((int)segs.size() > FDR_MAX_SEG) continue;
                // (k > 64: the merge stages every query's nseg * k keys in LDS)
                if (k > FDR_FAST_MAX_K && (int)segs.size() * k > FDR_MERGE_WIDE_CAP) continue;
                // (k > 1: the candidate pass, whose partial lists the workspace bound covers; the range pass, k = 1,
                // keeps no lists and wants many short segments when only a few query blocks are left)
                if (sh.tps > 0 && k > 1 && (int)segs.size() > (T + cap_tiles - 1) / cap_tiles + FDR_PLAN_EXTRA_SEG) continue;
                if (*std::max_element(segs.begin(), segs.end()) > cap_tiles) continue;
                const double cost = simulate_makespan(segs, p.nqb, slots, ov);
                if (cost < best_cost * 0.999) {
                    best_cost = cost;
                    best = segs;
                }
            }
    if (K.nseg > 0) {  // (development: that many equal segments)
        const int c = std::min(K.nseg, FDR_MAX_SEG);
        best.clear();
        const int l = (T + c - 1) / c;
        for (int left = T; left > 0; left -= l) best.push_back(std::min(left, l));
    }
    // Synchronised rounds (fp16 prefilter, more query blocks than resident slots).  With one launch for the
    // whole grid a finished workgroup is replaced at once, so after the first round the workgroups of an XCD
    // sit at unrelated positions of a segment and stream it through the XCD's 4 MB L2 one by one: 38 % L2 hit
    // rate, 850 GB of Infinity-Cache / HBM traffic per launch at 1 M rows against 0.2 GB of fp16 targets.  A
    // launch of at most `slots` workgroups starts them together on the same segment, they advance at the same
    // pace (their spread over a scan stays far inside the L2) and every tile is fetched once per XCD and
    // round.  One rank's slice of 1/8 of the queries -- a single such round -- ran 12.7 % faster per query
    // than the whole set before this.  Equal segments; their number trades the emptier last launch against
    // the per-launch cost.
    // Two queues (shapes with four workgroups per CU): launches of TWO workgroups per CU dealt alternately to two
    // queues, so two rounds are in flight and the workgroups of the next launch take the slots the stragglers
    // of the previous one have freed (one queue: every launch ends with its slowest workgroup while the rest
    // of the chip idles).  1 M rows: 124.9 -> 110.0 ms per step.  The launch size must be a multiple of the CU
    // count (448 or 576 workgroups instead of 512: +13...+18 %); three or four queues were slower.
    p.cohort = 0;
    p.queues = 1;
    const int wg_cu = std::max(1, knn_wg_per_cu(sh, k));
    int hw_slots = num_cus * wg_cu;
    const bool two_queues = K.streams < 0 || K.streams == 2;
    if (wg_cu >= 4 && two_queues) {
        p.queues = 2;
        hw_slots = num_cus * (wg_cu / 2);
    } else if ((wg_cu == 2 || (wg_cu == 1 && sh.tps >= 8)) && two_queues) {
        p.queues = 2;  // (d > 256, two workgroups per CU: full launches on two queues, 412 -> 389 ms at 2 M x 500;
                       // three workgroups per CU, d <= 256: one queue, no variant was faster)
    } else {
        p.queues = K.streams < 0 ? 1 : std::max(1, std::min(4, K.streams));
    }
    if (sh.tps == 0) {  // the exact kernel: rounds only when asked for (FDR_KNN_XROUNDS), full launches
        p.queues = K.xrounds == 2 ? 2 : 1;
        hw_slots = num_cus * wg_cu;
    }
    if (K.cohort_slots > 0) hw_slots = K.cohort_slots;
    const int cohort_mode = K.cohort;
    if (((sh.tps > 0 && sh.nq == 1) || (sh.tps == 0 && K.xrounds > 0)) && cohort_mode != 0 &&
        (p.nqb > num_cus * std::max(wg_cu, p.queues) || (cohort_mode == 2 && (long long)p.nqb * 2 > hw_slots))) {
        const int c0 = (T + cap_tiles - 1) / cap_tiles;
        double bc = 0.0;
        int bn = 0;
        for (int ns = c0; ns <= std::min(FDR_MAX_SEG, c0 + FDR_COHORT_EXTRA_SEG); ++ns) {
            const int len = (T + ns - 1) / ns;
            if (len < min_tiles && ns > c0) break;
            const long long items = (long long)p.nqb * ns;
            const long long launches = (items + hw_slots - 1) / hw_slots;
            const double cost = (double)launches * ((double)len + ov);
            if (bn == 0 || cost < bc * 0.999) {
                bc = cost;
                bn = ns;
            }
        }
        if (K.cohort_ns > 0) bn = K.cohort_ns;
        bn = std::max(c0, std::min(FDR_MAX_SEG, bn));
        const int len = (T + bn - 1) / bn;
        best.clear();
        for (int left = T; left > 0; left -= len) best.push_back(std::min(left, len));
        const long long items = (long long)p.nqb * (long long)best.size();
        const long long launches = (items + hw_slots - 1) / hw_slots;
        p.cohort = (int)((items + launches - 1) / launches);  // evenly filled launches
        if (p.queues > 1) p.cohort = std::min<long long>(hw_slots, items);  // (full launches: a multiple of the CU count)
    }
    if (p.cohort == 0) p.queues = 1;
    p.nseg = (int)best.size();
    int row = 0;
    for (int i = 0; i < p.nseg; ++i) {
        p.segs.b[i] = row;
        row += best[(size_t)i] * 32;
    }
    for (int i = p.nseg; i <= FDR_MAX_SEG; ++i) p.segs.b[i] = row;
    p.partial_bytes = (size_t)p.nseg * p.nq_pad * (size_t)k * sizeof(u64);
    p.bits_bytes = ((size_t)((nt + 31) / 32) * 4 + 255) / 256 * 256;
    p.shared_bytes = ((size_t)p.nq_pad * 4 + 255) / 256 * 256;
    p.total_bytes = p.bits_bytes + p.shared_bytes + p.partial_bytes;
    return p;
}


// ---- live-chunk groups of the d <= 128 candidate pass (knn_prefilter_live.inc) ---------------------------------------
// A 256-query block whose queries are all zero outside NL of the eight 16-component chunks runs on
// knn_prefilter_live_kernel<NL> (NL = 2 .. 6; a block with fewer live chunks is padded to 2); blocks with seven or eight
// live chunks keep the dense kernel.  The blocks of one instance form a group; a group's work items are (segment, block
// of the group), segment-major, and run in synchronised rounds of their own.  A group with fewer work items than
// `min_items` (one launch) joins the next larger NL -- the last live group joins the dense one -- and its blocks' ids are
// padded with chunks that are empty in the block, which is harmless: the kernel adds their true products, +0.
#define FDR_LIVE_MIN_NL 2
#define FDR_LIVE_MAX_NL 6
#define FDR_LIVE_DENSE 8  // LiveGroup::nl of the dense group
struct LiveGroup {
    int nl;            // chunks per tile the group's kernel multiplies (FDR_LIVE_DENSE: the dense kernel)
    int first, count;  // its blocks: order[first .. first + count), ascending
};
struct LivePlan {
    std::vector<int> order;       // every query block once, group by group
    std::vector<unsigned> ids;    // [block]: its group's nl chunk ids, ascending, four bits each (dense group: 0x76543210)
    std::vector<LiveGroup> groups;  // ascending nl; the dense group last
};
static int live_popcount8(unsigned m) {
    int c = 0;
    for (int b = 0; b < 8; ++b) c += (m >> b) & 1;
    return c;
}
// masks[b]: bit c set <=> chunk c is non-empty in some query of block b
static LivePlan live_plan(const unsigned *masks, int nqb, int nseg, long long min_items) {
    LivePlan P;
    P.order.reserve((size_t)nqb);
    P.ids.assign((size_t)nqb, 0x76543210u);
    std::vector<int> of_nl[FDR_LIVE_DENSE + 1];
    for (int b = 0; b < nqb; ++b) {
        const int pc = live_popcount8(masks[b] & 0xffu);
        of_nl[pc > FDR_LIVE_MAX_NL ? FDR_LIVE_DENSE : std::max(pc, FDR_LIVE_MIN_NL)].push_back(b);
    }
    for (int nl = FDR_LIVE_MIN_NL; nl <= FDR_LIVE_MAX_NL; ++nl) {  // small groups move up
        std::vector<int> &g = of_nl[nl];
        if (g.empty() || (long long)g.size() * nseg >= min_items) continue;
        std::vector<int> &up = of_nl[nl < FDR_LIVE_MAX_NL ? nl + 1 : FDR_LIVE_DENSE];
        std::vector<int> merged(g.size() + up.size());
        std::merge(g.begin(), g.end(), up.begin(), up.end(), merged.begin());
        up.swap(merged);
        g.clear();
    }
    for (int nl = FDR_LIVE_MIN_NL; nl <= FDR_LIVE_DENSE; ++nl) {
        const std::vector<int> &g = of_nl[nl];
        if (g.empty()) continue;
        P.groups.push_back(LiveGroup{nl, (int)P.order.size(), (int)g.size()});
        for (int b : g) {
            P.order.push_back(b);
            if (nl == FDR_LIVE_DENSE) continue;
            unsigned m = masks[b] & 0xffu;
            for (int c = 0; c < 8 && live_popcount8(m) < nl; ++c) m |= 1u << c;  // pad with the lowest empty chunks
            unsigned packed = 0;
            for (int c = 0, i = 0; c < 8; ++c)
                if ((m >> c) & 1) packed |= (unsigned)c << (4 * i++);
            P.ids[(size_t)b] = packed;
        }
    }
    return P;
}

// The order the pass issues a plan's groups in (indices into LivePlan::groups).  Ascending NL ends the pass on the
// dense group, whose work items last longest: behind the last launches no later launch takes the freed slots, so the
// chip drains for about one item time.  Descending -- the dense group first, NL = 6 down to the smallest -- ends it on
// the cheapest items instead (fdr_set_pass_tail; docs/experiments.md A-36).  The groups share no bound words and no
// lists, so the order changes no result.
static std::vector<int> live_issue_order(const LivePlan &P, bool descending) {
    std::vector<int> o(P.groups.size());
    for (size_t i = 0; i < o.size(); ++i) o[i] = (int)(descending ? o.size() - 1 - i : i);
    return o;
}

// ---- the launches of a pass: one list for every k-NN pass (fedrann_hip.hip: launch_rounds) ---------------------------
// A pass is one or more groups of work items -- a plain pass: one group of nqb * nseg; the live-chunk pass: a group per
// LiveGroup, count * nseg each -- and every group runs in launches of at most `per_launch` items (0: one launch per
// group), ascending and contiguous, only its last one short.  The launches are dealt round-robin over `queues` queues
// in issue order, across the groups: launch i goes to queue i % queues.
struct RoundLaunch {
    int group, queue;
    int base, grid;  // the group's items [base, base + grid)
};
static std::vector<RoundLaunch> round_schedule(const std::vector<long long> &items, long long per_launch, int queues) {
    std::vector<RoundLaunch> S;
    for (size_t g = 0; g < items.size(); ++g) {
        const long long n = items[g], per = per_launch > 0 ? per_launch : n;
        for (long long base = 0; base < n; base += per)
            S.push_back(RoundLaunch{(int)g, (int)(S.size() % (size_t)queues), (int)base, (int)std::min(per, n - base)});
    }
    return S;
}

// Work that depends on ONE group -- the merge and re-rank of its queries -- need not wait for the pass: it may be queued
// on a further stream once the group's last launch has been issued, behind an event on every queue.  Returns, per group,
// the index of the launch in front of which that happens, or -1: the group's work stays behind the join (always the
// group issued last, and a group without items).
//   FDR_TAIL_TRIGGER_GROUP: right behind the group's own last launch;
//   FDR_TAIL_TRIGGER_LAST:  in front of the final launch of every queue (the last `queues` launches of the list), for
//                           the groups that are complete by then: the work lands in the pass's tail, not all over it.
enum { FDR_TAIL_TRIGGER_NONE = 0, FDR_TAIL_TRIGGER_LAST = 1, FDR_TAIL_TRIGGER_GROUP = 2 };
static std::vector<int> round_ready_points(const std::vector<RoundLaunch> &S, size_t ngroups, int queues, int trigger) {
    std::vector<int> at(ngroups, -1), last(ngroups, -1);
    if (trigger == FDR_TAIL_TRIGGER_NONE || S.empty()) return at;
    for (size_t i = 0; i < S.size(); ++i) last[(size_t)S[i].group] = (int)i;
    const int cut = (int)S.size() - std::min<int>(queues, (int)S.size());
    for (size_t g = 0; g < ngroups; ++g) {
        if (last[g] < 0 || (int)g == S.back().group) continue;
        if (trigger == FDR_TAIL_TRIGGER_GROUP) at[g] = last[g] + 1;
        else if (last[g] < cut) at[g] = cut;
    }
    return at;
}
