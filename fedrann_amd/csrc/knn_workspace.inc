// Part of libfedrann_hip.so (included by fedrann_hip.hip after knn_plan.inc) and of the host-only sanitizer build
// (tests/host_san/host_san.cpp): the ONE description of the workspace of a k-NN call -- which regions it holds, of
// which element type and length, in which order, and which regions deliberately reuse another.  Plain C++, no HIP.
//
// A layout function walks an arena and fills a struct whose members are the typed pointers; with a null base the same
// walk only counts, and its `total` is what fdr_knn_workspace_bytes reports.
#ifdef __HIPCC__
typedef _Float16 ws_half;
typedef int4 ws_int4;
#else  // (the host-only build: stand-ins of the same size)
typedef uint16_t ws_half;
struct ws_int4 {
    int x, y, z, w;
};
#endif

#define RANGE_CAP 1024  // targets the range pass collects per query (knn_prefilter.inc); beyond it: the exact kernel
static_assert(RANGE_CAP == FDR_RANGE_CAP, "fdr_last_range_sets's row length (include/fedrann_hip.h)");
#define FDR_DEDUP_PROBE_BELOW (1 << 18)  // targets from which launch_knn skips the duplicate probe

static size_t align256(size_t x) { return (x + 255) / 256 * 256; }

struct WsRegion {
    size_t off, bytes;
};
struct WsArena {
    char *base;                              // null: count only
    std::vector<WsRegion> *log = nullptr;    // (the layout test: every region taken)
    size_t at = 0;
    template <class T>
    T *take(size_t count) {  // `count` elements of T at the current offset; the next region starts 256-byte aligned
        const size_t off = at;
        at += align256(count * sizeof(T));
        if (log) log->push_back({off, count * sizeof(T)});
        return base ? reinterpret_cast<T *>(base + off) : nullptr;
    }
};
// element n of a region, as the start of an alias inside it (null in a counting walk)
template <class T>
static T *ws_at(T *region, size_t n) { return region ? region + n : nullptr; }

// The three regions of a KnnPlan's p.total_bytes at `base`: the targets' zero bits, the query blocks' shared bound
// words, the per-segment partial lists -- for the exact pass and the candidate pass alike.
struct PlanRegions {
    unsigned *bits, *shared;
    u64 *partial;
};
static PlanRegions plan_regions(void *base, const KnnPlan &p) {
    char *const b = static_cast<char *>(base);
    return {reinterpret_cast<unsigned *>(b), reinterpret_cast<unsigned *>(b + p.bits_bytes),
            reinterpret_cast<u64 *>(b + p.bits_bytes + p.shared_bytes)};
}

// what a layout depends on besides the problem's size: the device, the context's modes, and the temporary storage
// rocprim asks for (fedrann_hip.hip: order_sort_tmp_bytes, class_tables_tmp_bytes; the layout test: stand-ins)
struct WsEnv {
    int num_cus, knn_mode, dedup_mode;
    size_t (*order_sort_tmp)(size_t rows);    // radix sort of `rows` (u64, int) pairs over 40 key bits
    size_t (*class_tables_tmp)(size_t rows);  // the larger of: radix sort of `rows` pairs over 64 bits, inclusive int scan
    int live_mode = FDR_LIVE_AUTO;            // fdr_set_live_chunks
    int compact_mode = FDR_COMPACT_AUTO;      // fdr_set_rerank_compact
};

// The compact records of the target rows (to_half_compact_kernel writes them, knn_rerank_kernel reads them;
// DESIGN.md section 5).  One record of RC_HALVES 64-byte halves per row; half h holds entries RC_HALF_ENTRIES * h ..
// of the row's non-zero components in canonical-chain order: byte 1 + e the position of entry e in the row as stored,
// the float at byte 16 + 4 e its value; byte 0 of half 0 is the row's number of non-zeros, and a count above
// RC_ENTRIES marks the row long (no entry of such a record is used).  A half is loaded whole; bytes the count does not
// cover are never used (the position is masked, the fmaf predicated off), so they may hold anything.
#ifndef RC_HALVES
#define RC_HALVES 2  // (1: the 64-byte form; docs/experiments.md A-32 has both forms' numbers)
#endif
#define RC_HALF_ENTRIES 12
#define RC_ENTRIES (RC_HALF_ENTRIES * RC_HALVES)
#define RC_BYTES (64 * RC_HALVES)
#define RC_DP 128  // the one width the records serve: positions are bytes
// FDR_COMPACT_AUTO_ON: whether AUTO builds and reads the records where the width allows -- decided by measurement,
// docs/experiments.md A-32.
#define FDR_COMPACT_AUTO_ON 1
static bool rerank_compact_wanted(int compact_mode, int dp) {  // are the records built?
    if (compact_mode == FDR_COMPACT_OFF || dp != RC_DP) return false;
    return compact_mode == FDR_COMPACT_FORCE || FDR_COMPACT_AUTO_ON;
}
// ... and read: under AUTO only while at most one target row in RC_LONG_SHARE is long.  A query of ~23 needed candidates
// then has no long one, and skips the dense route, about every second time; at 100 k reads (17.8 % long rows) nearly every
// query ran both routes and the step lost 1 % (A-32).
#define RC_LONG_SHARE 32
// The test is knn_rerank_kernel's own, on the count the build left on the device: n_long <= nt / RC_LONG_SHARE.

// The live-chunk candidate pass (knn_prefilter_live.inc).  FDR_LIVE_AUTO_ON: whether AUTO takes it where it applies --
// decided by measurement, docs/experiments.md A-22: 96.5 -> 70.9 ms per step at 1 M reads, so it does.
#define FDR_LIVE_AUTO_ON 1
// the candidate pass's shape: FORCE puts every d <= 128, K' <= 32 call on the eight-wave four-unit shape
static int prefilter_shape_live(int live_mode, int dp, int kp, int64_t nq, int num_cus, int64_t nt) {
    if (live_mode == FDR_LIVE_FORCE && dp == 128 && kp <= 32) return FDR_P128_W8U4;
    return prefilter_shape(dp, kp, nq, num_cus, nt);
}
// ... and whether a call of that shape and plan groups its query blocks by live chunks: only where the shipped
// eight-wave shape runs in synchronised rounds on two queues (FORCE: wherever the shape was forced)
static bool live_chunks_wanted(int live_mode, int shape, const KnnPlan &pp) {
    if (live_mode == FDR_LIVE_OFF || shape != FDR_P128_W8U4) return false;
    return live_mode == FDR_LIVE_FORCE || (FDR_LIVE_AUTO_ON && pp.cohort > 0 && pp.queues == 2);
}

// Stage skipping of the live-chunk pass (live_stage_masks_kernel, live_stage_lists_kernel; DESIGN.md section 6).  A
// stage is 128 ordered rows counted from its segment's first row; the tables are laid out in "stage rows", one per
// stage and two spare ones per segment, so that the place of segment g's tables follows from its first row alone:
// two segments' first rows that lie S stages apart differ by at least S - 1 in (row >> 7).
// FDR_SKIP_AUTO_ON: whether AUTO walks the lists -- decided by measurement, docs/experiments.md A-26.
#define FDR_SKIP_AUTO_ON 1
static FDR_HOST_DEVICE inline int live_stage_row(int t_begin, int seg) { return (t_begin >> 7) + 2 * seg; }
// the list of one mask value takes an even number of 16-bit entries: every list starts on a 32-bit word
static FDR_HOST_DEVICE inline int live_list_stride(int nstages) { return (nstages + 1) & ~1; }
static size_t live_stage_rows(int64_t nt) { return (size_t)(nt >> 7) + 2 * FDR_MAX_SEG + 2; }

// mode: FDR_MODE_AUTO uses the fp16 prefilter whenever it applies (d <= 512, k + 8 <= 64) and the target set is large
// enough to pay for it; fdr_set_knn_mode / FDR_KNN_MODE=exact|prefilter override it.
static bool knn_prefilter_wanted(int knn_mode, int64_t nt, int k) {
    if (knn_mode == FDR_MODE_EXACT) return false;
    const int kp = (k + prefilter_extra(k) + 1) & ~1;
    if (!(kp <= FDR_FAST_MAX_K && nt >= kp)) return false;
    if (nt > (int64_t)FDR_MAX_SEG << FDR_PREFILTER_MAX_IB) return false;  // segments too long for the keys
    return knn_mode == FDR_MODE_PREFILTER || nt >= 8192;
}

static bool knn_dedup_wanted(int dedup_mode, int64_t nq, int64_t nt) {
    if (dedup_mode != FDR_DEDUP_AUTO) return dedup_mode != FDR_DEDUP_OFF;
    return nt >= 8192 && nq >= 1024;  // (from the size at which the prefilter mode engages)
}

// Is searching nu unique targets for nuq unique queries worth the gathers and the expansion?  Never with fewer unique
// rows than neighbours asked for; else when forced (tests), or when the pairs to score fall to 90 %.
static bool dedup_worth(int nu, int nuq, int64_t nt, int64_t nq, int k, int dedup_mode) {
    if (nu < k) return false;
    return dedup_mode == FDR_DEDUP_FORCE || (double)nu * nuq <= 0.9 * (double)nt * (double)nq;
}

// ---- prefilter mode: fp16 pass -> certificate + exact re-rank -> exact pass for the rest ------------------------------
struct PrefilterWs {
    int kp, chunk, rchunk;
    int ordered;  // ordered scan possible: sort keys, order tables, ordered fp16 copies
    size_t knn_bytes, otmp_bytes, total;
    char *knn;  // knn_bytes shared (in stream order) by the candidate pass and the exact passes: a KnnPlan's regions
    ws_half *ht, *hq;  // fp16 targets, queries
    u64 *cand;         // [nq, kp] merged candidate keys
    int *counter;      // 1024 bytes: [0] exact list, [1] all-zero queries, [2] range list; inside it, the all-zero
    int *zidx;         // ... queries' one answer: k indices at + 256 bytes
    float *zdist;      // ... and k distances at + 512 bytes  (k <= FDR_FAST_MAX_K = 64)
    int *flagged;      // the exact list
    float *qc;         // chunked exact fall-back: the chunk's queries, zero flags, results
    uint8_t *qzc;
    int32_t *idxc;
    float *distc;
    int *rlist;  // range pass: its queries, their thresholds; per launch of rchunk queries: fp16 rows, thresholds,
    float *theta;  // counts, rows found
    ws_half *hqc;
    float *thetac;
    int *cnt, *rcand;
    uint8_t *path;  // per-query path codes (fdr_last_query_paths)
    // ordered only (else null); keys, values and sort scratch serve the targets, then the queries
    u64 *okeys, *okeys_s;
    int *ovals, *perm_t, *perm_q;
    ws_half *ho_t, *ho_q;
    char *otmp;
    // live-chunk pass only (else null): the ordered fp16 targets in blocks of (tile, chunk), the query blocks' chunk
    // masks, and the plan made from them (live_plan: blocks group by group, chunk ids per block)
    int live;
    ws_half *hb_t;
    unsigned *live_masks, *live_ids;
    int *live_order;
    // ... the stage-skip tables: per stage row the OR of its rows' masks; per (segment, block mask value 0 .. 255) the
    // ascending list of the segment's stages a block of that mask walks -- 256 lists of live_list_stride(stages) 16-bit
    // entries from entry 256 * live_stage_row(segment) on -- and their lengths [segment][mask value]
    uint8_t *live_smask;
    uint16_t *live_lists;
    int *live_lens;
    // ... and the dense group's queries side by side (the shipped kernel takes a block RANGE): rows, order table, bounds
    ws_half *live_hq;
    int *live_perm;
    unsigned *live_tau;
    // compact re-rank only (else null): one RC_BYTES record per target row; its build counts the long rows in
    // counter[8] (zeroed with the other counters, read back with them)
    uint8_t *rc;
};

static PrefilterWs prefilter_ws(const WsEnv &env, void *base, int64_t nq, int64_t nt, int d, int k,
                                std::vector<WsRegion> *log = nullptr) {
    PrefilterWs L = {};
    WsArena A{static_cast<char *>(base), log};
    L.kp = (k + prefilter_extra(k) + 1) & ~1;
    L.chunk = (int)std::min<int64_t>(nq, 16384);
    L.rchunk = (int)std::min<int64_t>(nq, 32768);  // range pass: queries per launch
    const size_t exact_all = knn_plan(env.num_cus, nq, nt, d, k).total_bytes;
    const int dp = padded_dim(d);
    const int pshape = prefilter_shape_live(env.live_mode, dp, L.kp, nq, env.num_cus, nt);
    const KnnPlan pp = knn_plan(env.num_cus, nq, nt, d, L.kp, pshape);
    // (a later call on fewer unique rows may plan more, shorter segments: room for the largest such plan)
    // (the bound words and the lists padded for the widest query block: a later call may choose the other shape)
    const size_t pre = std::max(pp.total_bytes, pp.bits_bytes + align256((size_t)(nq + 512) * 4) +
                                                    prefilter_partial_bound(nq, nt, L.kp, pp.qw));
    // any exact plan for <= chunk queries: bits + bound words + at most FDR_MAX_SEG segments of lists
    const size_t chunk_bound = align256((size_t)((nt + 31) / 32) * 4) + align256((size_t)(L.chunk + 128) * 4) +
                               (size_t)FDR_MAX_SEG * (L.chunk + 128) * (size_t)k * 8;
    L.knn_bytes = align256(std::max(exact_all, std::max(pre, chunk_bound)));
    L.knn = A.take<char>(L.knn_bytes);
    L.ht = A.take<ws_half>((size_t)nt * dp);
    L.hq = A.take<ws_half>((size_t)nq * dp);
    L.cand = A.take<u64>((size_t)nq * L.kp);
    L.counter = A.take<int>(256);
    L.zidx = ws_at(L.counter, 64);
    L.zdist = reinterpret_cast<float *>(ws_at(L.counter, 128));
    L.flagged = A.take<int>((size_t)nq);
    L.qc = A.take<float>((size_t)L.chunk * dp);
    L.qzc = A.take<uint8_t>((size_t)L.chunk);
    L.idxc = A.take<int32_t>((size_t)L.chunk * k);
    L.distc = A.take<float>((size_t)L.chunk * k);
    L.rlist = A.take<int>((size_t)nq);
    L.theta = A.take<float>((size_t)nq);
    L.hqc = A.take<ws_half>((size_t)L.rchunk * dp);
    L.thetac = A.take<float>((size_t)L.rchunk);
    L.cnt = A.take<int>((size_t)L.rchunk);
    L.rcand = A.take<int>((size_t)L.rchunk * RANGE_CAP);
    L.path = A.take<uint8_t>((size_t)nq);
    L.live = live_chunks_wanted(env.live_mode, pshape, pp);
    // (the sizes at which the pass runs in synchronised rounds; the live-chunk pass needs the order)
    L.ordered = pp.cohort > 0 || dev_knobs().ordered != 0 || L.live;
    if (L.ordered) {
        const size_t nmax = (size_t)std::max(nq, nt);
        L.okeys = A.take<u64>(nmax);
        L.okeys_s = A.take<u64>(nmax);
        L.ovals = A.take<int>(nmax);
        L.perm_t = A.take<int>((size_t)nt);
        L.perm_q = A.take<int>((size_t)nq);
        L.ho_t = A.take<ws_half>((size_t)nt * dp);
        L.ho_q = A.take<ws_half>((size_t)nq * dp);
        L.otmp_bytes = align256(env.order_sort_tmp(nmax));
        L.otmp = A.take<char>(L.otmp_bytes);
    }
    if (L.live) {
        // whole tiles of 32 rows, and four tiles more: a segment's last stage fetches up to three tiles past its end
        L.hb_t = A.take<ws_half>(((size_t)(nt + 31) / 32 + 4) * 32 * dp);
        const size_t nqb = (size_t)(nq + 255) / 256;
        L.live_masks = A.take<unsigned>(nqb);
        L.live_ids = A.take<unsigned>(nqb);
        L.live_order = A.take<int>(nqb);
        L.live_smask = A.take<uint8_t>(live_stage_rows(nt));
        L.live_lists = A.take<uint16_t>(live_stage_rows(nt) * 256);
        L.live_lens = A.take<int>((size_t)FDR_MAX_SEG * 256);
        L.live_hq = A.take<ws_half>(nqb * 256 * dp);
        L.live_perm = A.take<int>(nqb * 256);
        L.live_tau = A.take<unsigned>(nqb * 256);
    }
    if (rerank_compact_wanted(env.compact_mode, dp)) L.rc = A.take<uint8_t>((size_t)nt * RC_BYTES);
    L.total = A.at;
    return L;
}

// the workspace of launch_knn_mode: the prefilter mode's, or the exact pass's plan alone
static size_t knn_mode_workspace_bytes(const WsEnv &env, int64_t nq, int64_t nt, int d, int k) {
    if (knn_prefilter_wanted(env.knn_mode, nt, k)) return prefilter_ws(env, nullptr, nq, nt, d, k).total;
    return knn_plan(env.num_cus, nq, nt, d, k).total_bytes;
}

// ---- duplicate-row classes: search unique queries x unique targets, expand --------------------------------------------
struct DedupWs {
    size_t inner_bytes, tmp_bytes, total;
    char *inner;  // inner_bytes: workspace of the inner k-NN call (sized for the un-deduplicated problem)
    // One block: the sorted hashes follow the unsorted ones, and rep_m -- the (representative, size, start) table of
    // expand_classes_kernel, 16 bytes per unique row -- takes the place of both once the classes are marked (nothing
    // reads the hashes after that).
    u64 *hash, *hash_s;
    ws_int4 *rep_m;
    int *idx, *idx_s, *flag, *cid, *cls, *cstart, *isrep, *upos, *uofc, *cofu, *uqflag, *uqpos;
    float *U;  // the unique rows
    // Below FDR_DEDUP_PROBE_BELOW targets, and while U is still unused: a hash table of probe_slots (a power of two,
    // >= 2 nt) words and its duplicate counter behind it.  probe_slots = 0: U has no room for them, no probe.
    unsigned probe_slots;
    u64 *probe_table;
    int *probe_count;
    uint8_t *uzero;
    float *Uq;  // the unique queries (where they are not all the unique rows)
    uint8_t *uqz;
    int32_t *idx_u;  // the inner call's results
    float *dist_u;
    uint8_t *rowpath;  // path codes of the original rows (fdr_last_query_paths)
    char *tmp;         // tmp_bytes of rocprim scratch
};

static DedupWs dedup_ws(const WsEnv &env, void *base, int64_t nq, int64_t nt, int d, int k,
                        std::vector<WsRegion> *log = nullptr) {
    DedupWs L = {};
    WsArena A{static_cast<char *>(base), log};
    const int dp = padded_dim(d);
    const size_t n = (size_t)nt, hash_words = align256(n * 8) / 8;
    L.inner_bytes = align256(knn_mode_workspace_bytes(env, nq, nt, d, k));
    L.inner = A.take<char>(L.inner_bytes);
    L.hash = A.take<u64>(hash_words + n);
    L.hash_s = ws_at(L.hash, hash_words);
    L.rep_m = reinterpret_cast<ws_int4 *>(L.hash);  // (n x 16 bytes <= the block's)
    L.idx = A.take<int>(n);
    L.idx_s = A.take<int>(n);
    L.flag = A.take<int>(n);
    L.cid = A.take<int>(n);
    L.cls = A.take<int>(n);
    L.cstart = A.take<int>(n + 1);
    L.isrep = A.take<int>(n);
    L.upos = A.take<int>(n);
    L.uofc = A.take<int>(n);
    L.cofu = A.take<int>(n);
    L.uqflag = A.take<int>(n);
    L.uqpos = A.take<int>(n);
    L.U = A.take<float>(n * dp);
    if (nt < FDR_DEDUP_PROBE_BELOW) {
        unsigned tsize = 1024;
        while (tsize < 2u * (unsigned)n) tsize <<= 1;
        if ((size_t)tsize * 8 + 256 <= n * dp * 4) {
            L.probe_slots = tsize;
            L.probe_table = reinterpret_cast<u64 *>(L.U);
            L.probe_count = reinterpret_cast<int *>(ws_at(L.probe_table, tsize));
        }
    }
    L.uzero = A.take<uint8_t>(n);
    L.Uq = A.take<float>((size_t)nq * dp);
    L.uqz = A.take<uint8_t>((size_t)nq);
    L.idx_u = A.take<int32_t>((size_t)nq * k);
    L.dist_u = A.take<float>((size_t)nq * k);
    L.rowpath = A.take<uint8_t>((size_t)nq);
    L.tmp_bytes = align256(env.class_tables_tmp(n));
    L.tmp = A.take<char>(L.tmp_bytes);
    L.total = A.at;
    return L;
}

// fdr_knn_workspace_bytes for valid sizes
static size_t knn_workspace_bytes(const WsEnv &env, int64_t nq, int64_t nt, int d, int k) {
    const int route = knn_route(padded_dim(d), k, nt);
    if (route == FDR_ROUTE_GENERIC) return 256;  // (the generic kernel needs no scratch)
    if (route == FDR_ROUTE_WIDE) return knn_plan(env.num_cus, nq, nt, d, k).total_bytes;  // (the exact pass alone)
    if (knn_dedup_wanted(env.dedup_mode, nq, nt)) return dedup_ws(env, nullptr, nq, nt, d, k).total;
    return knn_mode_workspace_bytes(env, nq, nt, d, k);
}
