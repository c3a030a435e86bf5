// Host-only build of the library's plain-C++ parts under AddressSanitizer + UBSan (never the GPU build):
//   kmer_output_loader.inc (output.bin -> CSR), projection_tables.inc (the embed kernel's lookup tables),
//   csr_compact.inc (dead-feature filter), host_upload.inc (the pipelined upload's scheduler), knn_plan.inc (launch
//   planner), knn_workspace.inc (the workspace of a k-NN call), overlaps_writer.inc (overlaps.tsv).
// tests/test_host_san.py builds this with g++ -fsanitize=address,undefined and drives it; each command
// prints a result line that the test compares with what libfedrann_hip.so returns for the same input.  It builds it a
// second time with -fsanitize=thread and runs `upload`, the one case with threads that share state without a lock.
//
//   host_san loader PATH N_FEATURES THREADS       -> "rc=<code> R=.. nnz=.. sums=<4 weighted sums>" | "rc=<code> err=<msg>"
//   host_san loader-stale PATH N_FEATURES         -> load with capacities that no longer match: must fail cleanly
//   host_san tables SEED N_FEATURES D             -> builds tables for a random very-sparse P, checks them, compacts a CSR
//   host_san floats N  (hex float32 words on stdin) -> the writer's text of each
//   host_san overlaps OUT THREADS                 -> writes a random neighbour graph (whole, and as two appended blocks)
//   host_san plan-print NQ NT D K SHAPE           -> one plan (devtools)
//   host_san plan                                 -> sweeps the planner over edge sizes, checks invariants
//   host_san layout                               -> sweeps the k-NN workspace layouts (and plan_regions) over the same sizes, checks them
//   host_san upload                               -> sweeps the upload's scheduler over inputs x helper counts x links
//                                                    on a link that records what it is handed, checks the record
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/fedrann_hip.h"
#include "../../fedrann_amd/csrc/host_common.inc"
#include "../../fedrann_amd/csrc/knn_plan.inc"
#include "../../fedrann_amd/csrc/knn_workspace.inc"
#include "../../fedrann_amd/csrc/projection_tables.inc"
#include "../../fedrann_amd/csrc/csr_compact.inc"
#include "../../fedrann_amd/csrc/host_upload.inc"
#include "../../fedrann_amd/csrc/kmer_output_loader.inc"
#include "../../fedrann_amd/csrc/reads_parser.inc"
#include "../../fedrann_amd/csrc/overlaps_writer.inc"

template <typename T>
static uint64_t wsum(const std::vector<T> &v) {  // sum of (i + 1) * v[i] mod 2^64 (numpy can restate it)
    uint64_t s = 0;
    for (size_t i = 0; i < v.size(); ++i)
        s += (uint64_t)(i + 1) * (uint64_t)(typename std::make_unsigned<T>::type)v[i];
    return s;
}

static int cmd_loader(const char *path, long long F, int threads, bool stale) {
    int64_t R = 0, nnz = 0, nb = 0;
    int rc = fdr_kmer_output_scan(path, &R, &nnz, &nb);
    if (rc) {
        printf("rc=%d err=%s\n", rc, g_err);
        return 0;
    }
    std::vector<int64_t> indptr((size_t)(2 * R + 1)), name_off((size_t)(R + 1));
    std::vector<int32_t> indices((size_t)(2 * nnz));
    std::vector<char> names((size_t)nb);
    rc = fdr_kmer_output_load(path, F, threads, stale ? R + 1 : R, nnz, nb, indptr.data(), indices.data(),
                              name_off.data(), names.data());
    if (rc) {
        printf("rc=%d err=%s\n", rc, g_err);
        return 0;
    }
    printf("rc=0 R=%lld nnz=%lld sums=%llu,%llu,%llu,%llu\n", (long long)R, (long long)nnz,
           (unsigned long long)wsum(indptr), (unsigned long long)wsum(indices), (unsigned long long)wsum(name_off),
           (unsigned long long)wsum(names));
    return 0;
}

// records [lo, hi) through the ranged loader, arrays sized EXACTLY (an overrun is an ASan report)
static int cmd_loader_range(const char *path, long long F, int threads, long long lo, long long hi, int with_names) {
    int64_t R = 0, nnz = 0, nb = 0;
    int rc = fdr_kmer_output_scan_range(path, lo, hi, &R, &nnz, &nb);
    if (rc) {
        printf("rc=%d err=%s\n", rc, g_err);
        return 0;
    }
    std::vector<int64_t> indptr((size_t)(2 * (hi - lo) + 1)), name_off(with_names ? (size_t)(R + 1) : 0);
    std::vector<int32_t> indices((size_t)(2 * nnz));
    std::vector<char> names(with_names ? (size_t)nb : 0);
    rc = fdr_kmer_output_load_range(path, F, threads, R, lo, hi, nnz, nb, indptr.data(), indices.data(),
                                    with_names ? name_off.data() : nullptr, with_names ? names.data() : nullptr);
    if (rc) {
        printf("rc=%d err=%s\n", rc, g_err);
        return 0;
    }
    printf("rc=0 R=%lld nnz=%lld sums=%llu,%llu,%llu,%llu\n", (long long)R, (long long)nnz,
           (unsigned long long)wsum(indptr), (unsigned long long)wsum(indices), (unsigned long long)wsum(name_off),
           (unsigned long long)wsum(names));
    return 0;
}

// a FASTA / FASTQ file streamed in pieces of `chunk` bytes through fdr_reads_scan / fdr_reads_parse, every array
// sized EXACTLY (an overrun is an ASan report); the records go back out through fdr_kmer_output_append with one
// "index" per record (its sequence length), which exercises the writer under the sanitizers as well
static int cmd_reads(const char *path, long long chunk, int ids_as_fasta, const char *out_path) {
    FILE *f = fopen(path, "rb");
    if (!f) return 1;
    std::vector<uint8_t> buf;
    size_t have = 0;
    bool eof = false;
    int is_fastq = -1;
    long long n_rec = 0, n_bases = 0;
    unsigned long long s_seq = 0, s_ids = 0;
    {
        FILE *o = fopen(out_path, "wb");
        if (!o) return 1;
        const unsigned char hdr[16] = {'K', 'M', 'E', 'R', 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        fwrite(hdr, 1, 16, o);
        fclose(o);
    }
    while (!eof) {
        std::vector<uint8_t> piece(have + (size_t)chunk);  // (a fresh, exactly sized buffer per piece)
        if (have) memcpy(piece.data(), buf.data(), have);
        const size_t got = fread(piece.data() + have, 1, (size_t)chunk, f);
        piece.resize(have + got);
        eof = got < (size_t)chunk;
        if (is_fastq < 0) is_fastq = !piece.empty() && piece[0] == '@';
        int64_t used = 0, R = 0, nb = 0;
        int rc = fdr_reads_scan(piece.data(), (int64_t)piece.size(), is_fastq, ids_as_fasta, eof ? 1 : 0, &used, &R, &nb);
        if (rc) {
            printf("rc=%d err=%s\n", rc, g_err);
            return 0;
        }
        std::vector<uint8_t> seqs((size_t)nb);
        std::vector<int64_t> off((size_t)R + 1), span((size_t)(2 * R));
        rc = fdr_reads_parse(piece.data(), used, is_fastq, ids_as_fasta, R, nb, seqs.data(), off.data(), span.data());
        if (rc) {
            printf("rc=%d err=%s\n", rc, g_err);
            return 0;
        }
        std::vector<int64_t> name_off((size_t)R + 1, 0), indptr((size_t)R + 1, 0);
        std::vector<char> names;
        std::vector<int32_t> idx((size_t)R);
        for (int64_t r = 0; r < R; ++r) {
            for (int64_t i = span[(size_t)(2 * r)]; i < span[(size_t)(2 * r + 1)]; ++i) {
                s_ids = s_ids * 1099511628211ull + piece[(size_t)i];
                names.push_back((char)(piece[(size_t)i] < 32 || piece[(size_t)i] > 126 ? '?' : piece[(size_t)i]));
            }
            s_ids = s_ids * 1099511628211ull + 255;
            name_off[(size_t)r + 1] = (int64_t)names.size();
            idx[(size_t)r] = (int32_t)(off[(size_t)r + 1] - off[(size_t)r]);
            indptr[(size_t)r + 1] = r + 1;
        }
        for (uint8_t c : seqs) s_seq = s_seq * 1099511628211ull + c;
        rc = fdr_kmer_output_append(out_path, R, name_off.data(), names.data(), indptr.data(), idx.data());
        if (rc) {
            printf("rc=%d err=%s\n", rc, g_err);
            return 0;
        }
        n_rec += R;
        n_bases += nb;
        buf.assign(piece.begin() + used, piece.end());
        have = buf.size();
    }
    fclose(f);
    printf("rc=0 R=%lld bases=%lld seq=%llu ids=%llu\n", n_rec, n_bases, s_seq, s_ids);
    return 0;
}

static int cmd_tables(unsigned seed, long long F, int d) {
    std::mt19937_64 rng(seed);
    // a very sparse P: each feature row is non-empty with probability ~ d / sqrt(F) (capped), 1-3 entries
    std::vector<int64_t> indptr((size_t)F + 1, 0);
    std::vector<int32_t> cols;
    std::vector<float> vals;
    const double p = std::min(0.5, (double)d / std::sqrt((double)F));
    for (long long f = 0; f < F; ++f) {
        if ((rng() >> 11) * (1.0 / 9007199254740992.0) < p) {
            const int n = 1 + (int)(rng() % 3);
            for (int i = 0; i < n; ++i) {
                cols.push_back((int32_t)(rng() % (unsigned)d));
                vals.push_back((float)((int)(rng() % 2001) - 1000) / 256.0f);
            }
        }
        indptr[(size_t)f + 1] = (int64_t)cols.size();
    }
    ProjectionTables T;
    int rc = build_projection_tables(F, d, indptr.data(), cols.data(), vals.data(), T);
    if (rc) {
        printf("rc=%d err=%s\n", rc, g_err);
        return 1;
    }
    // invariants: bit <=> non-empty row, prefix counts, rowinfo mirrors the CSR
    unsigned rows = 0;
    for (long long f = 0; f < F; ++f) {
        const bool bit = (T.ftab[(size_t)(f >> 5)].x >> (f & 31)) & 1u;
        const bool nonempty = indptr[(size_t)f + 1] > indptr[(size_t)f];
        if (bit != nonempty) return printf("FAIL bit %lld\n", f), 1;
        if ((f & 31) == 0 && T.ftab[(size_t)(f >> 5)].y != rows) return printf("FAIL prefix %lld\n", f), 1;
        if (nonempty) {
            const PU4 &ri = T.rowinfo[rows++];
            if (ri.x != (unsigned)indptr[(size_t)f] || ri.y != (unsigned)(indptr[(size_t)f + 1] - indptr[(size_t)f]) ||
                ri.z != (unsigned)cols[(size_t)indptr[(size_t)f]])
                return printf("FAIL rowinfo %lld\n", f), 1;
        }
    }
    if (rows != T.rows) return printf("FAIL rows\n"), 1;
    // bad inputs must be refused, not read out of bounds
    {
        std::vector<int64_t> bad = indptr;
        bad[(size_t)F / 2] = bad[(size_t)F] + 5;
        ProjectionTables U;
        if (build_projection_tables(F, d, bad.data(), cols.data(), vals.data(), U) == FDR_OK) return printf("FAIL monotone\n"), 1;
        if (!cols.empty()) {
            std::vector<int32_t> bc = cols;
            bc[bc.size() / 2] = d;
            if (build_projection_tables(F, d, indptr.data(), bc.data(), vals.data(), U) == FDR_OK) return printf("FAIL column\n"), 1;
        }
        if (build_projection_tables(F, FDR_MAX_DIM + 1, indptr.data(), cols.data(), vals.data(), U) == FDR_OK) return printf("FAIL dim\n"), 1;
    }
    // compaction of a random CSR (incl. empty rows, ids outside [0, F)) at 1 and 5 threads == a serial filter
    std::vector<uint32_t> bits(T.ftab.size());
    for (size_t w = 0; w < bits.size(); ++w) bits[w] = T.ftab[w].x;
    const int64_t n_rows = 20000;
    std::vector<int64_t> a_ip((size_t)n_rows + 1, 0);
    std::vector<int32_t> a_ix;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int n = (r % 97 == 0) ? 0 : (int)(rng() % 300);
        std::vector<int32_t> row;
        for (int i = 0; i < n; ++i) row.push_back((int32_t)(rng() % (uint64_t)(F + (r % 1013 == 0 ? 7 : 0))));
        std::sort(row.begin(), row.end());
        a_ix.insert(a_ix.end(), row.begin(), row.end());
        a_ip[(size_t)r + 1] = (int64_t)a_ix.size();
    }
    std::vector<int64_t> want_ip((size_t)n_rows + 1, 0);
    std::vector<int32_t> want_ix;
    for (int64_t r = 0; r < n_rows; ++r) {
        for (int64_t q = a_ip[(size_t)r]; q < a_ip[(size_t)r + 1]; ++q) {
            const int64_t f = a_ix[(size_t)q];
            if (f < F && indptr[(size_t)f + 1] > indptr[(size_t)f]) want_ix.push_back((int32_t)f);
        }
        want_ip[(size_t)r + 1] = (int64_t)want_ix.size();
    }
    for (int threads : {1, 5}) {
        std::vector<int64_t> o_ip((size_t)n_rows + 1);
        std::vector<int32_t> o_ix(want_ix.size());  // exactly enough room: one more write would be caught
        rc = csrc::compact(bits, F, n_rows, a_ip.data(), a_ix.data(), o_ip.data(), o_ix.data(), (int64_t)o_ix.size(), threads);
        if (rc || o_ip != want_ip || o_ix != want_ix) return printf("FAIL compact threads=%d rc=%d\n", threads, rc), 1;
        // the chunk form of the pipelined upload (host_upload.inc; AVX-512 rows where the CPU has them): any row range
        for (int64_t c0 = 0; c0 < n_rows; c0 += 97) {
            const int64_t c1 = std::min<int64_t>(n_rows, c0 + 97), raw = a_ip[(size_t)c1] - a_ip[(size_t)c0];
            std::vector<int32_t> buf((size_t)raw + 16);
            std::vector<int64_t> ptr((size_t)(c1 - c0) + 1);
            const int64_t n = csrc::compact_chunk(bits.data(), (uint64_t)F, a_ip.data(), a_ix.data(), c0, c1, buf.data(), raw, ptr.data());
            if (n != want_ip[(size_t)c1] - want_ip[(size_t)c0]) return printf("FAIL compact_chunk count at row %lld\n", (long long)c0), 1;
            for (int64_t r = c0; r <= c1; ++r)
                if (ptr[(size_t)(r - c0)] != want_ip[(size_t)r] - want_ip[(size_t)c0]) return printf("FAIL compact_chunk pointers\n"), 1;
            if (n > 0 && memcmp(buf.data(), want_ix.data() + want_ip[(size_t)c0], (size_t)n * 4) != 0) return printf("FAIL compact_chunk ids\n"), 1;
            if (raw > 0 && csrc::compact_chunk(bits.data(), (uint64_t)F, a_ip.data(), a_ix.data(), c0, c1, buf.data(), raw - 1, ptr.data()) != -1 &&
                n == raw)
                return printf("FAIL compact_chunk capacity\n"), 1;
        }
        if (!want_ix.empty() &&
            csrc::compact(bits, F, n_rows, a_ip.data(), a_ix.data(), o_ip.data(), o_ix.data(), (int64_t)o_ix.size() - 1, threads) == FDR_OK)
            return printf("FAIL capacity\n"), 1;
    }
    printf("rc=0 rows=%u nnz=%zu kept=%zu of %zu\n", T.rows, cols.size(), want_ix.size(), a_ix.size());
    return 0;
}

// pass: the family of the pass that runs the plan (FDR_FAM_TILE, _PREFILTER or _RANGE; the ping-pong forms count as theirs)
static int check_plan(int cus, int64_t nq, int64_t nt, int d, int k, int shape, int pass) {
    const KnnPlan p = knn_plan(cus, nq, nt, d, k, shape);
    const KnnShape &sh = kShapes[p.shape];
    const int T = (int)((nt + 31) / 32);
    bool ok = p.nseg >= 1 && p.nseg <= FDR_MAX_SEG && p.segs.b[0] == 0 && p.qw == 32 * sh.nq * sh.nw &&
              (int64_t)p.nqb * p.qw >= nq && p.nq_pad == p.nqb * p.qw;
    for (int i = 0; i < p.nseg && ok; ++i) {
        const int len = p.segs.b[i + 1] - p.segs.b[i];
        ok = len > 0 && len % 32 == 0 && (sh.tps == 0 || len <= (1 << FDR_PREFILTER_MAX_IB));
    }
    ok = ok && p.segs.b[p.nseg] == T * 32;
    for (int i = p.nseg; i <= FDR_MAX_SEG && ok; ++i) ok = p.segs.b[i] == T * 32;
    ok = ok && p.cohort >= 0 && (p.cohort == 0 || (p.cohort <= cus * 4 && sh.tps > 0)) &&
         p.total_bytes == p.bits_bytes + p.shared_bytes + p.partial_bytes &&
         p.partial_bytes == (size_t)p.nseg * p.nq_pad * (size_t)k * 8;
    // a shape the default knobs choose is compiled into the release library, as a kernel of the pass's family (the
    // candidate pass: for the list width K' = k needs)
    const bool family = sh.family == pass || (pass == FDR_FAM_PREFILTER && sh.family == FDR_FAM_PINGPONG) ||
                        (pass == FDR_FAM_RANGE && sh.family == FDR_FAM_RANGE_PP);
    ok = ok && sh.release && family && (pass != FDR_FAM_PREFILTER || (sh.lists & (k <= 32 ? 16 : 32)));
    if (!ok) printf("FAIL plan cus=%d nq=%lld nt=%lld d=%d k=%d shape=%d nseg=%d\n", cus, (long long)nq, (long long)nt, d, k, shape, p.nseg);
    return ok ? 0 : 1;
}

static int cmd_plan() {
    int bad = 0, n = 0;
    const int64_t sizes[] = {20, 64, 8191, 8192, 8193, 100000, (1 << 19) - 1, 1 << 19, (1 << 19) + 1, 1000000,
                             1250000, 2500000, 10000000, 20000000, ((int64_t)FDR_MAX_SEG << FDR_PREFILTER_MAX_IB)};
    for (int cus : {256, 304, 64})
        for (int64_t nt : sizes)
            for (int d : {16, 128, 256, 500})
                for (int k : {1, 20, 50, 64}) {
                    if (nt < k) continue;
                    const int dp = padded_dim(d);
                    for (int64_t nq : {nt, (nt + 7) / 8, (int64_t)1}) {
                        bad += check_plan(cus, nq, nt, d, k, -1, FDR_FAM_TILE);  // exact shapes
                        ++n;
                        const int kp = (k + prefilter_extra(k) + 1) & ~1;
                        if (kp <= FDR_FAST_MAX_K && nt >= kp) {
                            bad += check_plan(cus, nq, nt, d, kp, prefilter_shape(dp, kp, nq, cus), FDR_FAM_PREFILTER);
                            bad += check_plan(cus, nq, nt, d, kp, prefilter_shape(dp, kp, nq, cus, nt), FDR_FAM_PREFILTER);
                            bad += check_plan(cus, nq, nt, d, 1, range_shape(dp), FDR_FAM_RANGE);
                            // the range pass's chunks: a few plateau queries, or all of them
                            for (const int64_t plateau : {std::min<int64_t>(nq, 4095), nq}) {
                                const int c = (int)std::min<int64_t>(plateau, 32768);
                                bad += check_plan(cus, c, nt, d, 1, range_shape(dp, c, (int)plateau), FDR_FAM_RANGE);
                            }
                            n += 5;
                        }
                    }
                }
    // configs 4 / 5 of BASELINE.json: one rank's plan must fit FDR_MAX_SEG segments
    const KnnPlan c4 = knn_plan(256, 1250000, 10000000, 128, 28, prefilter_shape(128, 28, 1250000, 256));
    const KnnPlan c5 = knn_plan(256, 2500000, 20000000, 256, 58, prefilter_shape(256, 58, 2500000, 256));
    printf("rc=%d plans=%d config4_nseg=%d config5_nseg=%d\n", bad ? 1 : 0, n, c4.nseg, c5.nseg);
    return bad ? 1 : 0;
}

// ---- the k-NN workspace layouts (knn_workspace.inc) on a fake base: nothing is read or written through the pointers
struct LayoutCheck {
    const char *base;
    size_t total;
    const std::vector<WsRegion> &log;
    bool ok = true;
    // every region 256-byte aligned, inside [base, base + total), and disjoint from every other
    void regions() {
        std::vector<WsRegion> r = log;
        std::sort(r.begin(), r.end(), [](const WsRegion &a, const WsRegion &b) { return a.off < b.off; });
        for (size_t i = 0; i < r.size(); ++i) {
            ok = ok && r[i].off % 256 == 0 && r[i].off + r[i].bytes <= total;
            ok = ok && (i == 0 || r[i - 1].off + r[i - 1].bytes <= r[i].off);
        }
    }
    // `region` is one of the regions taken, and `alias` [bytes] lies inside it, from `from` bytes into it onwards
    void inside(const void *alias, size_t bytes, const void *region, size_t from = 0) {
        const size_t ro = (size_t)((const char *)region - base), ao = (size_t)((const char *)alias - base);
        bool found = false;
        for (const WsRegion &r : log)
            if (r.off == ro) found = ao >= ro + from && ao + bytes <= ro + r.bytes;
        ok = ok && alias && region && found;
    }
};

// plan_regions: a plan's three regions -- zero bits, bound words, partial lists -- lie inside p.total_bytes, 256-byte
// aligned and disjoint
static bool check_plan_regions(const KnnPlan &p, int64_t nt) {
    char *const base = reinterpret_cast<char *>((uintptr_t)1 << 40);
    const PlanRegions R = plan_regions(base, p);
    const std::vector<WsRegion> log = {{(size_t)((char *)R.bits - base), (size_t)((nt + 31) / 32) * 4},
                                       {(size_t)((char *)R.shared - base), (size_t)p.nq_pad * 4},
                                       {(size_t)((char *)R.partial - base), p.partial_bytes}};
    LayoutCheck c{base, p.total_bytes, log};
    c.regions();
    return c.ok && (char *)R.bits == base;
}

static size_t g_tmp_bytes;  // what the stand-ins for rocprim's temporary-storage queries answer
static size_t tmp_standin(size_t) { return g_tmp_bytes; }

static int check_layouts(const WsEnv &env, int64_t nq, int64_t nt, int d, int k) {
    char *const base = reinterpret_cast<char *>((uintptr_t)1 << 40);
    const int dp = padded_dim(d);
    bool ok = true;
    size_t want = knn_plan(env.num_cus, nq, nt, d, k).total_bytes;  // what fdr_knn_workspace_bytes must say
    ok = ok && check_plan_regions(knn_plan(env.num_cus, nq, nt, d, k), nt);  // (the exact pass's plan)
    if (knn_prefilter_wanted(env.knn_mode, nt, k)) {
        std::vector<WsRegion> log;
        const PrefilterWs L = prefilter_ws(env, base, nq, nt, d, k, &log);
        // (the candidate pass's plan, as launch_knn_prefilter asks for it)
        ok = ok && check_plan_regions(knn_plan(env.num_cus, nq, nt, d, L.kp, prefilter_shape_live(env.live_mode, dp, L.kp, nq, env.num_cus, nt)), nt);
        LayoutCheck c{base, L.total, log};
        c.regions();
        c.inside(L.zidx, (size_t)k * 4, L.counter, 16);  // (the three counters come first)
        c.inside(L.zdist, (size_t)k * 4, L.counter, 16);
        ok = c.ok && (const char *)L.zidx + (size_t)k * 4 <= (const char *)L.zdist && L.knn == base;
        ok = ok && prefilter_ws(env, nullptr, nq, nt, d, k).total == L.total && L.knn_bytes <= L.total;
        ok = ok && L.chunk >= 1 && L.chunk <= nq && L.rchunk >= 1 && L.rchunk <= nq && L.kp >= k && (L.ordered != 0) == (L.otmp != nullptr);
        // the regions of every plan that runs in the shared head: the candidate pass, the whole exact fall-back, and the
        // chunked one for any c <= chunk queries
        ok = ok && L.knn_bytes >= knn_plan(env.num_cus, nq, nt, d, k).total_bytes &&
             L.knn_bytes >= knn_plan(env.num_cus, nq, nt, d, L.kp, prefilter_shape(dp, L.kp, nq, env.num_cus, nt)).total_bytes;
        for (const int64_t cq : {(int64_t)1, (int64_t)127, (int64_t)129, (int64_t)L.chunk / 2, (int64_t)L.chunk - 1, (int64_t)L.chunk})
            if (cq >= 1 && cq <= L.chunk) ok = ok && L.knn_bytes >= knn_plan(env.num_cus, cq, nt, d, k).total_bytes;
        want = L.total;
    }
    ok = ok && knn_mode_workspace_bytes(env, nq, nt, d, k) == want;
    if (knn_dedup_wanted(env.dedup_mode, nq, nt)) {
        std::vector<WsRegion> log;
        const DedupWs W = dedup_ws(env, base, nq, nt, d, k, &log);
        LayoutCheck c{base, W.total, log};
        c.regions();
        const size_t n = (size_t)nt;
        c.inside(W.hash_s, n * 8, W.hash, n * 8);  // (behind the unsorted hashes: the sort reads one and writes the other)
        c.inside(W.rep_m, n * 16, W.hash);
        if (W.probe_slots) {
            c.inside(W.probe_table, (size_t)W.probe_slots * 8, W.U);
            c.inside(W.probe_count, 4, W.U, (size_t)W.probe_slots * 8);
            ok = ok && W.probe_slots >= 2 * n && (W.probe_slots & (W.probe_slots - 1)) == 0 && nt < FDR_DEDUP_PROBE_BELOW;
        }
        ok = ok && c.ok && W.inner == base && dedup_ws(env, nullptr, nq, nt, d, k).total == W.total;
        ok = ok && W.inner_bytes >= want && W.tmp_bytes >= g_tmp_bytes;  // (the inner call on the full problem)
        want = W.total;
    }
    ok = ok && knn_workspace_bytes(env, nq, nt, d, k) == want;
    if (!ok)
        printf("FAIL layout cus=%d mode=%d dedup=%d tmp=%zu nq=%lld nt=%lld d=%d k=%d\n", env.num_cus, env.knn_mode,
               env.dedup_mode, g_tmp_bytes, (long long)nq, (long long)nt, d, k);
    return ok ? 0 : 1;
}

// the sizes of cmd_plan on the route that has these workspaces (FDR_ROUTE_FAST), every k-NN mode x duplicate-row mode
static int cmd_layout() {
    int bad = 0, n = 0;
    const int64_t sizes[] = {20, 64, 8191, 8192, 8193, 100000, (1 << 19) - 1, 1 << 19, (1 << 19) + 1, 1000000,
                             1250000, 2500000, 10000000, 20000000, ((int64_t)FDR_MAX_SEG << FDR_PREFILTER_MAX_IB)};
    for (const size_t tmp : {(size_t)0, (size_t)1, (size_t)3 << 20}) {
        g_tmp_bytes = tmp;
        for (int cus : {256, 304, 64})
            for (int64_t nt : sizes)
                for (int d : {16, 128, 256, 500})
                    for (int k : {1, 20, 50, 64}) {
                        if (nt < k || knn_route(padded_dim(d), k, nt) != FDR_ROUTE_FAST) continue;
                        for (int64_t nq : {nt, (nt + 7) / 8, (int64_t)1})
                            for (int mode : {FDR_MODE_AUTO, FDR_MODE_EXACT, FDR_MODE_PREFILTER})
                                for (int dedup : {FDR_DEDUP_AUTO, FDR_DEDUP_OFF, FDR_DEDUP_FORCE}) {
                                    bad += check_layouts(WsEnv{cus, mode, dedup, tmp_standin, tmp_standin}, nq, nt, d, k);
                                    ++n;
                                }
                    }
    }
    printf("rc=%d layouts=%d\n", bad ? 1 : 0, n);
    return bad ? 1 : 0;
}

// ---- the pipelined upload's scheduler (host_upload.inc) on a stand-in link that records what it is handed
struct UploadInput {
    const char *name;
    std::vector<int64_t> ip;
    std::vector<int32_t> ix;
    std::vector<uint32_t> bits;
    int64_t F;
    int64_t n_rows() const { return (int64_t)ip.size() - 1; }
};

// rows of len(r) ascending ids below F (a few beyond it); every `alive_of`-th feature has a P row
template <typename LenFn>
static UploadInput upload_input(const char *name, std::mt19937_64 &rng, int64_t n_rows, int64_t F, int alive_of, LenFn &&len) {
    UploadInput in{name, std::vector<int64_t>((size_t)n_rows + 1, 0), {}, std::vector<uint32_t>((size_t)(F + 31) / 32, 0), F};
    for (int64_t f = 0; f < F; f += alive_of) in.bits[(size_t)(f >> 5)] |= 1u << (f & 31);
    for (int64_t r = 0; r < n_rows; ++r) {
        std::vector<int32_t> row((size_t)len(r));
        for (int32_t &f : row) f = (int32_t)(rng() % (uint64_t)(F + (r % 101 == 0 ? 7 : 0)));
        std::sort(row.begin(), row.end());
        in.ix.insert(in.ix.end(), row.begin(), row.end());
        in.ip[(size_t)r + 1] = (int64_t)in.ix.size();
    }
    return in;
}

struct RecordingLink {
    struct Raw {
        int64_t r0, r1;
        int slot;
    };
    const std::vector<int32_t> &stage_ids;
    const std::vector<int64_t> &stage_ptr;
    int sleep_us;  // what every send takes
    int stall_at;  // the raw send (by its number) that takes a tenth of a second on top, -1: none
    std::vector<Raw> raws;
    bool pending[2] = {false, false};
    bool slots_ok = true;  // a slot is waited for before it is used again: never more than two runs in flight
    int staged_sends = 0, ops = 0, staged_at = -1;
    int64_t first_row = -1, used = 0;
    std::vector<int32_t> ids;  // what the staged send took: the last `used` ids ...
    std::vector<int64_t> ptr;  // ... and stage_ptr[first_row .. n_rows]

    void take_time() const {
        if (sleep_us) std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
    }
    int send_raw(int64_t r0, int64_t r1, int slot) {
        if (slot >= 0) {
            slots_ok = slots_ok && slot < 2 && !pending[slot];
            pending[slot] = true;
        }
        if ((int)raws.size() == stall_at) std::this_thread::sleep_for(std::chrono::milliseconds(100));
        raws.push_back({r0, r1, slot});
        ++ops;
        take_time();
        return FDR_OK;
    }
    int wait_slot(int slot) {
        slots_ok = slots_ok && slot >= 0 && slot < 2 && pending[slot];
        pending[slot] = false;
        return FDR_OK;
    }
    int send_staged(int64_t first, int64_t n_used) {
        ++staged_sends;
        staged_at = ops++;
        first_row = first;
        used = n_used;
        if (n_used < 0 || n_used > (int64_t)stage_ids.size() || first < 0 || first >= (int64_t)stage_ptr.size()) return FDR_OK;  // (reported by the caller's checks)
        ids.assign(stage_ids.end() - n_used, stage_ids.end());
        ptr.assign(stage_ptr.begin() + first, stage_ptr.end());
        take_time();
        return FDR_OK;
    }
};

struct UploadTally {
    int combos = 0, staged = 0, overflow = 0, refused = 0;
    int met[3] = {0, 0, 0};  // runs of input "sparse" whose fronts met in the first, the middle, the last third of the rows
};

// one upload of `in` (malformed: some row breaks 0 <= indptr[r] <= indptr[r + 1] <= nnz and the call must refuse it) with
// `helpers` threads and a link that takes sleep_us per send and stalls once, after stall_share percent of the runs the
// input has (-1: never); every array sized EXACTLY (an overrun is an ASan report)
static int upload_once(const UploadInput &in, const hup::Tuning &tune, int helpers, int sleep_us, int stall_share, bool malformed,
                       UploadTally &tally) {
    const int64_t n_rows = in.n_rows(), nnz = in.ip[(size_t)n_rows], cap = std::max<int64_t>(64, nnz / 6);  // (staging as small as the chunks)
    std::vector<int32_t> stage_ids((size_t)cap, -1);
    std::vector<int64_t> stage_ptr((size_t)n_rows + 1, -7);
    const int64_t runs = ((int64_t)hup::cut_chunks(in.ip.data(), n_rows, tune.ids_per_chunk).size() + tune.run - 1) / tune.run;
    RecordingLink link{stage_ids, stage_ptr, sleep_us, stall_share < 0 ? -1 : (int)(runs * stall_share / 100)};
    hup::Outcome o;
    {
        hup::WorkerPool pool;  // (a pool of its own: helpers = 0 is "no thread could be started")
        o = hup::upload(tune, n_rows, in.ip.data(), in.ix.data(), in.bits.data(), (uint64_t)in.F, stage_ids.data(), stage_ptr.data(),
                        cap, pool, helpers, link);
    }
    auto failed = [&](const char *what) {
        printf("FAIL upload %s: %s (helpers=%d sleep=%d rc=%d bad_row=%lld)\n", in.name, what, helpers, sleep_us, o.rc, (long long)o.bad_row);
        return 1;
    };
    ++tally.combos;
    if (!link.slots_ok) return failed("a slot reused before it was waited for");
    if (malformed) {  // refused at a row that is malformed, whichever thread met it, and nobody was handed such a row's ids
        auto bad = [&](int64_t r) { return in.ip[(size_t)r] < 0 || in.ip[(size_t)r + 1] < in.ip[(size_t)r] || in.ip[(size_t)r + 1] > nnz; };
        if (o.rc != FDR_E_ARG || o.bad_row < 0 || o.bad_row >= n_rows || !bad(o.bad_row)) return failed("malformed indptr not refused at such a row");
        if (link.staged_sends) return failed("staged send of a refused input");
        for (const RecordingLink::Raw &s : link.raws)
            for (int64_t r = s.r0; r < s.r1; ++r)
                if (bad(r)) return failed("malformed row sent");
        ++tally.refused;
        return 0;
    }
    if (o.rc != FDR_OK || o.bad_row >= 0) return failed("valid input refused");
    // the link's view: raw runs of whole chunks from row 0 upwards, at most `run` chunks each, on alternating slots; then
    // at most one of: the staged send, one raw send (slot -1) of the rest
    const std::vector<hup::Chunk> chunks = hup::cut_chunks(in.ip.data(), n_rows, tune.ids_per_chunk);
    std::vector<int64_t> chunk_at((size_t)n_rows + 1, -1);  // row -> the chunk that starts there
    for (size_t c = 0; c < chunks.size(); ++c) chunk_at[(size_t)chunks[c].r0] = (int64_t)c;
    chunk_at[(size_t)n_rows] = (int64_t)chunks.size();
    int64_t next = 0;
    for (size_t i = 0; i < link.raws.size(); ++i) {
        const RecordingLink::Raw &s = link.raws[i];
        if (s.r0 != next || s.r1 <= s.r0 || s.r1 > n_rows) return failed("raw sends not contiguous");
        const int64_t c0 = chunk_at[(size_t)s.r0], c1 = chunk_at[(size_t)s.r1];
        if (c0 < 0 || c1 < 0) return failed("raw send not of whole chunks");
        if (s.slot >= 0 ? (s.slot != (int)(i & 1) || c1 - c0 > tune.run) : (i + 1 != link.raws.size() || s.r1 != n_rows || link.staged_sends))
            return failed("raw run too long, on the wrong slot, or a rest that is not last");
        next = s.r1;
    }
    if (link.staged_sends > 1 || (link.staged_sends == 1 && (link.first_row != next || link.staged_at != link.ops - 1)))
        return failed("staged send not once, last, from where the raw runs ended");
    if (link.staged_sends == 0 && next != n_rows) return failed("rows not covered");
    if (o.raw_rows != next || o.staged_rows != n_rows - next) return failed("outcome's row counts");
    // staged row pointers: ascending inside [cap - used, cap], from the first staged id to the end of the buffer
    if (link.staged_sends) {
        if (link.used < 0 || link.used > cap || (int64_t)link.ptr.size() != n_rows - next + 1) return failed("staged sizes");
        if (link.ptr.front() != cap - link.used || link.ptr.back() != cap) return failed("staged pointers' ends");
        for (size_t r = 0; r + 1 < link.ptr.size(); ++r)
            if (link.ptr[r] > link.ptr[r + 1]) return failed("staged pointers not ascending");
    }
    // per row, the ids the embed kernel meets (raw rows: filtered by the bitmap, as the kernel does) == csrc::compact
    std::vector<int64_t> want_ip((size_t)n_rows + 1);
    std::vector<int32_t> want_ix((size_t)nnz);
    if (csrc::compact(in.bits, in.F, n_rows, in.ip.data(), in.ix.data(), want_ip.data(), want_ix.data(), nnz, 1)) return failed("compact");
    for (int64_t r = 0; r < n_rows; ++r) {
        std::vector<int32_t> got;
        if (r < next) {
            for (int64_t q = in.ip[(size_t)r]; q < in.ip[(size_t)r + 1]; ++q) {
                const uint32_t f = (uint32_t)in.ix[(size_t)q];
                if ((int64_t)f < in.F && ((in.bits[f >> 5] >> (f & 31)) & 1u)) got.push_back((int32_t)f);
            }
        } else {
            const int64_t base = cap - link.used;
            got.assign(link.ids.begin() + (link.ptr[(size_t)(r - next)] - base), link.ids.begin() + (link.ptr[(size_t)(r - next) + 1] - base));
        }
        if (got != std::vector<int32_t>(want_ix.begin() + want_ip[(size_t)r], want_ix.begin() + want_ip[(size_t)r + 1]))
            return failed("a row's ids differ from csrc::compact");
    }
    tally.staged += link.staged_sends;
    tally.overflow += o.overflow ? 1 : 0;
    if (!strcmp(in.name, "sparse")) ++tally.met[std::min<int64_t>(2, 3 * next / n_rows)];
    return 0;
}

static int cmd_upload() {
    std::mt19937_64 rng(11);
    hup::Tuning tune;  // small chunks and staging, so that a few thousand rows are hundreds of chunks
    tune.ids_per_chunk = 96;
    auto some = [&](int64_t) { return (int)(rng() % 40); };
    std::vector<UploadInput> inputs;
    inputs.push_back(upload_input("sparse", rng, 4000, 5000, 20, some));  // the helpers' chunks fit the staging buffer
    inputs.push_back(upload_input("full", rng, 9000, 5000, 1, some));     // every id survives: staging overflows, the rest goes raw
    inputs.push_back(upload_input("empty-rows", rng, 6000, 5000, 10, [&](int64_t r) { return r < 50 || r % 1000 > 300 || r > 5900 ? 0 : (int)(rng() % 60); }));
    inputs.push_back(upload_input("long-row", rng, 3000, 5000, 10, [&](int64_t r) { return r % 700 == 350 ? 500 : (int)(rng() % 20); }));
    inputs.push_back(upload_input("one-row", rng, 1, 5000, 3, [](int64_t) { return 300; }));
    inputs.push_back(upload_input("few-rows", rng, 3, 5000, 3, [](int64_t r) { return r == 1 ? 0 : 150; }));
    const size_t n_valid = inputs.size();
    // a dip in indptr: at a chunk boundary, inside a chunk the link takes first, inside one of the helpers' end; and the two
    // other ways an entry can be wrong: negative, beyond the ids (a little, and by so much that adding to it overflows)
    const std::vector<hup::Chunk> cut = hup::cut_chunks(inputs[0].ip.data(), inputs[0].n_rows(), tune.ids_per_chunk);
    auto inside = [&](size_t c) {  // an indptr entry strictly inside a chunk at or after c
        while (cut[c].r1 - cut[c].r0 < 2) ++c;
        return (cut[c].r0 + cut[c].r1) / 2;
    };
    struct Dip {
        const char *name;
        int64_t entry, below_prev;  // indptr[entry] = indptr[entry - 1] - below_prev, or (below_prev = 0) a fixed value
        int64_t value;
    };
    const int64_t nnz0 = inputs[0].ip.back();
    const Dip dips[] = {{"dip-boundary", cut[cut.size() / 2].r0, 1, 0}, {"dip-front", inside(1), 1, 0}, {"dip-back", inside(cut.size() - 8), 1, 0},
                        {"negative", inside(cut.size() / 3), 0, -3}, {"beyond", inside(2 * cut.size() / 3), 0, nnz0 + 9},
                        {"huge", cut[cut.size() / 4].r0, 0, std::numeric_limits<int64_t>::max() - 5}};
    for (const Dip &d : dips) {
        UploadInput in = inputs[0];
        in.name = d.name;
        if (in.ip[(size_t)d.entry - 1] < 1) return printf("FAIL upload: no room for a dip\n"), 1;
        in.ip[(size_t)d.entry] = d.below_prev ? in.ip[(size_t)d.entry - 1] - d.below_prev : d.value;
        inputs.push_back(in);
    }
    UploadTally tally;
    // The links: an instant one; two that sleep per send (us), about as fast as the helpers and much slower; and two
    // instant ones that stall ONCE for a tenth of a second, before their first run and after half of the runs.  Where the
    // fronts meet is up to the scheduler (on an idle machine the woken helpers may take every chunk before the calling
    // thread's first claim), except at the ends: without helpers the link carries all rows (the back), and behind the stall
    // before the first run the helpers take all that is left (the front).
    const struct {
        int sleep_us, stall_share;
    } links[5] = {{0, -1}, {30, -1}, {1000, -1}, {0, 50}, {0, 0}};
    int bad = 0;
    for (size_t i = 0; i < inputs.size(); ++i)
        for (int helpers : {0, 1, 5, 15})
            for (int l = 0; l < 5; ++l)
                bad += upload_once(inputs[i], tune, helpers, links[l].sleep_us, links[l].stall_share, i >= n_valid, tally);
    printf("rc=%d combos=%d staged=%d overflow=%d refused=%d met=%d,%d,%d\n", bad ? 1 : 0, tally.combos, tally.staged, tally.overflow,
           tally.refused, tally.met[0], tally.met[1], tally.met[2]);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "upload") return cmd_upload();
    if (cmd == "loader" && argc == 5) return cmd_loader(argv[2], atoll(argv[3]), atoi(argv[4]), false);
    if (cmd == "loader-stale" && argc == 4) return cmd_loader(argv[2], atoll(argv[3]), 2, true);
    if (cmd == "loader-range" && argc == 8)
        return cmd_loader_range(argv[2], atoll(argv[3]), atoi(argv[4]), atoll(argv[5]), atoll(argv[6]), atoi(argv[7]));
    if (cmd == "reads" && argc == 6) return cmd_reads(argv[2], atoll(argv[3]), atoi(argv[4]), argv[5]);
    if (cmd == "tables" && argc == 5) return cmd_tables((unsigned)atoi(argv[2]), atoll(argv[3]), atoi(argv[4]));
    if (cmd == "plan") return cmd_plan();
    if (cmd == "layout") return cmd_layout();
    if (cmd == "floats" && argc == 3) {  // host_san floats N: float32 bit patterns (one hex word per line on stdin) -> text
        char line[64], out[64];
        long long n = atoll(argv[2]);
        while (n-- > 0 && fgets(line, sizeof(line), stdin)) {
            const uint32_t bits = (uint32_t)strtoul(line, nullptr, 16);
            float x;
            memcpy(&x, &bits, 4);
            const int len = ovw::format_float32(x, out);
            fwrite(out, 1, (size_t)len, stdout);
            fputc('\n', stdout);
        }
        return 0;
    }
    if (cmd == "overlaps" && argc == 4) {  // host_san overlaps OUT THREADS: a random graph incl. -1 fillers, self hits, inf
        std::mt19937_64 rng(7);
        const int64_t n = 3000;
        const int k = 11;
        std::vector<int64_t> off((size_t)n + 1, 0);
        std::string names;
        std::vector<uint8_t> strands((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            names += "read_" + std::to_string(i / 2) + std::string((size_t)(rng() % 5), 'x');
            if (i % 211 == 0) names += "\"q\"";  // (a name csv.QUOTE_MINIMAL quotes and doubles)
            if (i % 307 == 0) names += "\tz";
            off[(size_t)i + 1] = (int64_t)names.size();
            strands[(size_t)i] = (uint8_t)(i & 1);
        }
        std::vector<int32_t> idx((size_t)(n * k));
        std::vector<float> dist((size_t)(n * k));
        for (int64_t i = 0; i < n * k; ++i) {
            idx[(size_t)i] = (rng() % 50 == 0) ? -1 : (int32_t)(rng() % (uint64_t)n);
            const uint32_t bits = (uint32_t)(rng() % 0x3f800001u);  // [0, 1]
            memcpy(&dist[(size_t)i], &bits, 4);
            if (rng() % 97 == 0) dist[(size_t)i] = std::numeric_limits<float>::infinity();
            if (rng() % 389 == 0) dist[(size_t)i] = std::numeric_limits<float>::quiet_NaN();  // (an empty field)
        }
        for (int64_t q = 0; q < n; q += 3) idx[(size_t)(q * k)] = (int32_t)q;
        int64_t lines = 0, lines2 = 0;
        // whole graph in one call, then the same graph as two row blocks appended to a second file
        int rc = fdr_overlaps_write(argv[2], 0, 1, n, 0, n, k, idx.data(), dist.data(), off.data(), names.data(),
                                    strands.data(), atoi(argv[3]), &lines);
        const std::string p2 = std::string(argv[2]) + ".parts";
        int64_t l1 = 0;
        if (!rc) rc = fdr_overlaps_write(p2.c_str(), 0, 1, n, 0, 1000, k, idx.data(), dist.data(), off.data(), names.data(),
                                         strands.data(), atoi(argv[3]), &l1);
        if (!rc) rc = fdr_overlaps_write(p2.c_str(), 1, 0, n, 1000, n - 1000, k, idx.data() + 1000 * k, dist.data() + 1000 * k,
                                         off.data(), names.data(), strands.data(), atoi(argv[3]), &lines2);
        idx[5] = (int32_t)n;  // out of range: refused
        const int rc_bad = fdr_overlaps_write((std::string(argv[2]) + ".bad").c_str(), 0, 1, n, 0, n, k, idx.data(), dist.data(),
                                              off.data(), names.data(), strands.data(), 1, nullptr);
        printf("rc=%d lines=%lld parts=%lld bad_rc=%d\n", rc, (long long)lines, (long long)(l1 + lines2), rc_bad);
        return rc ? 1 : 0;
    }
    if (cmd == "plan-print" && argc == 7) {  // host_san plan-print NQ NT D K SHAPE  (shape -1: the exact mode's choice)
        const KnnPlan p = knn_plan(256, atoll(argv[2]), atoll(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
        printf("shape=%d nqb=%d nseg=%d cohort=%d queues=%d tiles:", p.shape, p.nqb, p.nseg, p.cohort, p.queues);
        for (int i = 0; i < p.nseg; ++i) printf(" %d", (p.segs.b[i + 1] - p.segs.b[i]) / 32);
        printf(" bytes=%zu\n", p.total_bytes);
        return 0;
    }
    fprintf(stderr, "usage: host_san loader|loader-stale|tables|plan|layout|upload ...\n");
    return 2;
}
