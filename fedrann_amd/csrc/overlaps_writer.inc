// Part of libfedrann_hip.so (included by fedrann_hip.hip) and of the host-only sanitizer build
// (tests/host_san/host_san.cpp).  Plain C++, no HIP.
//
// overlaps.tsv writer: replaces get_output_dataframe + DataFrame.to_csv(sep="\t", index=False)
// (fedrann/__main__.py:261-300, :385) -- an N x k Python loop that fills six lists, a DataFrame of object
// columns and pandas' CSV formatter: the end-to-end bottleneck once the k-NN runs on the GPU (N k = 2e7 .. 1e9
// lines).  Same bytes: header line, then for every row q and column r with target t = idx[q][r], in that
// order, unless t == q (the row itself; the other strand of the same read is kept):
//     name[q] \t "+-"[strand[q]] \t name[t] \t "+-"[strand[t]] \t r \t dist \n
// r keeps its column number; a negative t aliases from the end like Python indexing does (the reference's
// behaviour for pynndescent's -1 fillers); dist is float32 and pandas prints its shortest round-trip
// representation in numpy's layout: positional for 1e-4 <= |x| < 1e16 ("0.660664", "1.0"), else scientific
// with an exponent of at least two digits ("1.1920929e-07", "4e-22"), "inf"; a NaN distance is an empty field
// (pandas' na_rep).  Names go through csv.QUOTE_MINIMAL as to_csv applies it (Python 3.12, the reference's pin,
// lineterminator "\n"): a name that contains the separator, a double quote or a line feed is wrapped in double
// quotes with its quotes doubled; a carriage return alone does not quote.
// Blocks of rows are formatted by a pool of threads into private buffers and written in order.
#include <charconv>

namespace ovw {

// shortest round-trip digits of a positive finite float: returns the number of digits, sets the decimal
// exponent such that value = 0.d1d2d3... * 10^decpt
static int shortest_digits(float x, char *digits, int *decpt) {
    char buf[32];
    const std::to_chars_result r = std::to_chars(buf, buf + sizeof(buf), x, std::chars_format::scientific);
    // d[.ddd]e[+-]XX
    int n = 0;
    const char *p = buf;
    for (; p < r.ptr && *p != 'e'; ++p)
        if (*p != '.') digits[n++] = *p;
    int e = 0;
    if (p < r.ptr) {
        ++p;
        const bool neg = *p == '-';
        if (*p == '-' || *p == '+') ++p;
        for (; p < r.ptr; ++p) e = e * 10 + (*p - '0');
        if (neg) e = -e;
    }
    while (n > 1 && digits[n - 1] == '0') --n;  // (to_chars never pads, defensive)
    *decpt = e + 1;
    return n;
}

// numpy / pandas text of a float32 (see the header comment); returns the number of characters written
static int format_float32(float x, char *out) {
    char *o = out;
    if (x != x) return 0;  // NaN: pandas writes na_rep = "" for a missing value
    if (x < 0.0f || (x == 0.0f && std::signbit(x))) {
        *o++ = '-';
        x = -x;
    }
    if (x == std::numeric_limits<float>::infinity()) {
        memcpy(o, "inf", 3);
        return (int)(o - out) + 3;
    }
    if (x == 0.0f) {
        memcpy(o, "0.0", 3);
        return (int)(o - out) + 3;
    }
    char d[16];
    int decpt;
    const int n = shortest_digits(x, d, &decpt);
    const double xd = (double)x;  // (numpy compares the value as a double: float32(1e-4) < 1e-4, float32(1e16) > 1e16)
    if (xd >= 1e-4 && xd < 1e16) {  // positional
        if (decpt <= 0) {
            *o++ = '0';
            *o++ = '.';
            for (int i = 0; i < -decpt; ++i) *o++ = '0';
            memcpy(o, d, (size_t)n);
            o += n;
        } else if (decpt >= n) {
            memcpy(o, d, (size_t)n);
            o += n;
            for (int i = n; i < decpt; ++i) *o++ = '0';
            *o++ = '.';
            *o++ = '0';
        } else {
            memcpy(o, d, (size_t)decpt);
            o += decpt;
            *o++ = '.';
            memcpy(o, d + decpt, (size_t)(n - decpt));
            o += n - decpt;
        }
    } else {  // scientific: d[.ddd]e[+-]XX (no fraction for a single digit, at least two exponent digits)
        *o++ = d[0];
        if (n > 1) {
            *o++ = '.';
            memcpy(o, d + 1, (size_t)(n - 1));
            o += n - 1;
        }
        *o++ = 'e';
        int e = decpt - 1;
        *o++ = e < 0 ? '-' : '+';
        if (e < 0) e = -e;
        char eb[8];
        int en = 0;
        do {
            eb[en++] = (char)('0' + e % 10);
            e /= 10;
        } while (e);
        if (en < 2) eb[en++] = '0';
        while (en) *o++ = eb[--en];
    }
    return (int)(o - out);
}

static inline char *put_uint(char *o, unsigned v) {
    char b[12];
    int n = 0;
    do {
        b[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) *o++ = b[--n];
    return o;
}

// one name field under QUOTE_MINIMAL (see the header comment)
static inline void put_name(std::string &out, const char *p, size_t n) {
    bool special = false;
    for (size_t i = 0; i < n; ++i)
        if (p[i] == '\t' || p[i] == '"' || p[i] == '\n') {
            special = true;
            break;
        }
    if (!special) {
        out.append(p, n);
        return;
    }
    out.push_back('"');
    for (size_t i = 0; i < n; ++i) {
        if (p[i] == '"') out.push_back('"');
        out.push_back(p[i]);
    }
    out.push_back('"');
}

static const char kHeader[] = "query_name\tquery_orientation\ttarget_name\ttarget_orientation\tneighbor_rank\tdistance\n";

}  // namespace ovw

namespace ovw {

// fdr_overlaps_write (indptr == nullptr: row r's entries are [r k, (r + 1) k)) and fdr_overlaps_write_csr (row r's
// entries are [indptr[r], indptr[r + 1])): one body, one line formatter
static int write_rows(const char *who, const char *path, int32_t append, int32_t write_header, int64_t n_total,
                      int64_t row0, int64_t n_rows, int32_t k, const int64_t *indptr, const int32_t *idx,
                      const float *dist, const int64_t *name_off, const char *names, const uint8_t *strands,
                      int32_t n_threads, int64_t *lines_out) {
    if (!path || n_total <= 0 || row0 < 0 || n_rows < 0 || row0 + n_rows > n_total || k < 1 || !name_off)
        return fail(FDR_E_ARG, "%s: bad argument", who);
    int64_t n_entries = n_rows * (int64_t)k;
    if (indptr) {
        if (indptr[0] < 0) return fail(FDR_E_ARG, "%s: indptr[0] is negative", who);
        for (int64_t r = 0; r < n_rows; ++r)
            if (indptr[r + 1] < indptr[r]) return fail(FDR_E_ARG, "%s: indptr not monotone at row %lld", who, (long long)r);
        n_entries = indptr[n_rows] - indptr[0];
    }
    if (n_entries > 0 && (!idx || !dist)) return fail(FDR_E_ARG, "%s: bad argument", who);
    // strands == NULL: fwd / rev doubled rows as parse_kmer_searcher_output yields them (feature_extraction.py:136-140):
    // names / name_off describe the n_total / 2 RECORDS, row t carries record t >> 1's id and strand t & 1 -- the ids are
    // never materialised twice (10 M reads: 0.7 GB of id bytes per copy, per rank)
    const bool doubled = strands == nullptr;
    if (doubled && (n_total & 1)) return fail(FDR_E_ARG, "%s: doubled rows need an even row count", who);
    const int64_t n_names = doubled ? n_total / 2 : n_total;
    const int nshift = doubled ? 1 : 0;
    if (name_off[0] < 0 || (name_off[n_names] > 0 && !names)) return fail(FDR_E_ARG, "%s: bad names", who);
    for (int64_t i = 0; i < n_names; ++i)
        if (name_off[i + 1] < name_off[i]) return fail(FDR_E_ARG, "%s: name offsets not monotone at %lld", who, (long long)i);
    FILE *f = fopen(path, append ? "ab" : "wb");
    if (!f) return fail(FDR_E_IO, "cannot open %s for writing", path);
    if (write_header && fwrite(kHeader, 1, sizeof(kHeader) - 1, f) != sizeof(kHeader) - 1) {
        fclose(f);
        return fail(FDR_E_IO, "write to %s failed", path);
    }
    int nthr = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    nthr = std::max(1, std::min(nthr, 64));
    if (n_entries < (1 << 15)) nthr = 1;
    const int64_t BLOCK = 4096;  // rows per formatted block
    const int64_t nblocks = (n_rows + BLOCK - 1) / BLOCK;
    std::atomic<int64_t> bad{-1};
    int64_t lines = 0;
    int rc = FDR_OK;
    // rounds of nthr blocks: formatted in parallel, written in order
    std::vector<std::string> bufs((size_t)nthr);
    std::vector<int64_t> cnt((size_t)nthr, 0);
    for (int64_t b0 = 0; b0 < nblocks && rc == FDR_OK; b0 += nthr) {
        const int nb = (int)std::min<int64_t>(nthr, nblocks - b0);
        auto format_block = [&](int w) {
            std::string &out = bufs[(size_t)w];
            out.clear();
            int64_t made = 0;
            const int64_t r_lo = (b0 + w) * BLOCK, r_hi = std::min(n_rows, r_lo + BLOCK);
            char tail[64];
            for (int64_t r = r_lo; r < r_hi; ++r) {
                const int64_t q = row0 + r;
                const int64_t qi = q >> nshift;
                const char *qn = names + name_off[qi];
                const size_t ql = (size_t)(name_off[qi + 1] - name_off[qi]);
                const char qo = (doubled ? (int)(q & 1) : (int)strands[q]) ? '-' : '+';
                const int64_t e0 = indptr ? indptr[r] : r * (int64_t)k;
                const int64_t len = indptr ? indptr[r + 1] - e0 : (int64_t)k;
                for (int64_t c = 0; c < len; ++c) {
                    int64_t t = idx[e0 + c];
                    if (t == q) continue;
                    if (t < 0) t += n_total;  // Python's negative indexing (names[-1] is the last read)
                    if (t < 0 || t >= n_total) {
                        int64_t exp = -1;
                        bad.compare_exchange_strong(exp, q);
                        continue;
                    }
                    put_name(out, qn, ql);
                    out.push_back('\t');
                    out.push_back(qo);
                    out.push_back('\t');
                    const int64_t ti = t >> nshift;
                    put_name(out, names + name_off[ti], (size_t)(name_off[ti + 1] - name_off[ti]));
                    out.push_back('\t');
                    out.push_back((doubled ? (int)(t & 1) : (int)strands[t]) ? '-' : '+');
                    out.push_back('\t');
                    char *o = put_uint(tail, (unsigned)c);
                    *o++ = '\t';
                    o += format_float32(dist[e0 + c], o);
                    *o++ = '\n';
                    out.append(tail, (size_t)(o - tail));
                    ++made;
                }
            }
            cnt[(size_t)w] = made;
        };
        std::vector<std::thread> pool;
        try {
            for (int w = 1; w < nb; ++w) pool.emplace_back(format_block, w);
        } catch (...) {
            for (std::thread &t : pool) t.join();
            for (int w = (int)pool.size() + 1; w < nb; ++w) format_block(w);
            pool.clear();
        }
        format_block(0);
        for (std::thread &t : pool) t.join();
        for (int w = 0; w < nb && rc == FDR_OK; ++w) {
            const std::string &s = bufs[(size_t)w];
            if (!s.empty() && fwrite(s.data(), 1, s.size(), f) != s.size()) rc = fail(FDR_E_IO, "write to %s failed", path);
            lines += cnt[(size_t)w];
        }
    }
    if (fclose(f) != 0 && rc == FDR_OK) rc = fail(FDR_E_IO, "closing %s failed", path);
    if (rc == FDR_OK && bad.load() >= 0)
        rc = fail(FDR_E_ARG, "%s: row %lld has a neighbour index outside [-%lld, %lld)", who, (long long)bad.load(),
                  (long long)n_total, (long long)n_total);
    if (lines_out) *lines_out = lines;
    return rc;
}

}  // namespace ovw

FDR_EXPORT int fdr_overlaps_write(const char *path, int32_t append, int32_t write_header, int64_t n_total,
                                  int64_t row0, int64_t n_rows, int32_t k, const int32_t *idx, const float *dist,
                                  const int64_t *name_off, const char *names, const uint8_t *strands, int32_t n_threads,
                                  int64_t *lines_out) {
    return ovw::write_rows("overlaps_write", path, append, write_header, n_total, row0, n_rows, k, nullptr, idx, dist,
                           name_off, names, strands, n_threads, lines_out);
}

// The ragged form: row r's entries are idx / dist [indptr[r], indptr[r + 1]) (the result of a radius search)
FDR_EXPORT int fdr_overlaps_write_csr(const char *path, int32_t append, int32_t write_header, int64_t n_total,
                                      int64_t row0, int64_t n_rows, const int64_t *indptr, const int32_t *idx,
                                      const float *dist, const int64_t *name_off, const char *names,
                                      const uint8_t *strands, int32_t n_threads, int64_t *lines_out) {
    if (!indptr) return fail(FDR_E_ARG, "overlaps_write_csr: bad argument");
    return ovw::write_rows("overlaps_write_csr", path, append, write_header, n_total, row0, n_rows, 1, indptr, idx,
                           dist, name_off, names, strands, n_threads, lines_out);
}
