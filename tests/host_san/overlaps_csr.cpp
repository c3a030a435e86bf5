// The ragged overlaps writer (fdr_overlaps_write_csr, overlaps_writer.inc), HOST-ONLY under AddressSanitizer + UBSan:
// tests/test_overlaps_csr_host.py builds this with the flags of test_host_san.py and runs it.
//   overlaps_csr DIR THREADS  -> writes random ragged graphs (arrays sized EXACTLY: an overrun is an ASan report) whole,
//                                as appended blocks and in the doubled-rows mode; checks the blocks against the whole
//                                file, a CSR of equal-length rows against fdr_overlaps_write, the refusals; prints
//                                "rc=0 lines=<data lines> cases=<graphs>"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fedrann_hip.h"
#include "../../fedrann_amd/csrc/host_common.inc"
#include "../../fedrann_amd/csrc/overlaps_writer.inc"

static std::string slurp(const std::string &path) {
    std::string s;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return s;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("rc=1 failed=%s line=%d err=%s\n", #cond, __LINE__, g_err); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: overlaps_csr DIR THREADS\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int threads = atoi(argv[2]);
    std::mt19937_64 rng(7);
    long long total_lines = 0;
    int cases = 0;
    for (int doubled = 0; doubled < 2; ++doubled)
        for (int64_t n : {2, 10, 5000, 20000}) {
            // names of the rows (doubled: of the n / 2 records), some of them needing quotes
            const int64_t n_names = doubled ? n / 2 : n;
            std::vector<int64_t> name_off((size_t)n_names + 1, 0);
            std::string names;
            for (int64_t i = 0; i < n_names; ++i) {
                names += "read_" + std::to_string(i);
                if (i % 97 == 3) names += "\t\"q\"";
                name_off[(size_t)i + 1] = (int64_t)names.size();
            }
            std::vector<uint8_t> strands((size_t)n);
            for (auto &s : strands) s = (uint8_t)(rng() & 1);
            // ragged rows: empty ones, self first / in the middle / last, a negative index now and then
            std::vector<int64_t> indptr((size_t)n + 1, 0);
            std::vector<int32_t> idx;
            std::vector<float> dist;
            for (int64_t r = 0; r < n; ++r) {
                const int len = (rng() % 5 == 0) ? 0 : (int)(rng() % 9);
                const int self_at = len ? (int)(rng() % (uint64_t)len) : -1;
                for (int c = 0; c < len; ++c) {
                    int64_t t = (int64_t)(rng() % (uint64_t)n);
                    if (c == self_at && r % 3 != 0) t = r;
                    if (rng() % 50 == 0) t = -1 - (int64_t)(rng() % (uint64_t)n);
                    idx.push_back((int32_t)t);
                    dist.push_back((float)(rng() % 1000) / 1024.0f * (rng() % 7 == 0 ? 1e-6f : 1.0f));
                }
                indptr[(size_t)r + 1] = (int64_t)idx.size();
            }
            idx.shrink_to_fit();
            dist.shrink_to_fit();
            const uint8_t *st = doubled ? nullptr : strands.data();
            const std::string whole = dir + "/whole.tsv", parts = dir + "/parts.tsv";
            int64_t lines = 0;
            CHECK(fdr_overlaps_write_csr(whole.c_str(), 0, 1, n, 0, n, indptr.data(), idx.data(), dist.data(),
                                         name_off.data(), names.data(), st, threads, &lines) == 0);
            total_lines += lines;
            // three appended blocks, each with an indptr and arrays of its own
            int64_t part_lines = 0;
            const int64_t cuts[4] = {0, n / 3, n / 3 + (n > 2 ? 1 : 0), n};
            for (int b = 0; b < 3; ++b) {
                const int64_t lo = cuts[b], hi = cuts[b + 1];
                std::vector<int64_t> ip((size_t)(hi - lo) + 1);
                for (int64_t r = lo; r <= hi; ++r) ip[(size_t)(r - lo)] = indptr[(size_t)r] - indptr[(size_t)lo];
                std::vector<int32_t> bi(idx.begin() + indptr[(size_t)lo], idx.begin() + indptr[(size_t)hi]);
                std::vector<float> bd(dist.begin() + indptr[(size_t)lo], dist.begin() + indptr[(size_t)hi]);
                int64_t got = -1;
                CHECK(fdr_overlaps_write_csr(parts.c_str(), b > 0, b == 0, n, lo, hi - lo, ip.data(), bi.data(), bd.data(),
                                             name_off.data(), names.data(), st, threads, &got) == 0);
                part_lines += got;
            }
            CHECK(part_lines == lines);
            CHECK(slurp(whole) == slurp(parts));
            // rows of one length: the fixed-width writer's bytes
            const int k = 5;
            std::vector<int64_t> kp((size_t)n + 1);
            for (int64_t r = 0; r <= n; ++r) kp[(size_t)r] = r * k;
            std::vector<int32_t> ki((size_t)(n * k));
            std::vector<float> kd((size_t)(n * k));
            for (size_t i = 0; i < ki.size(); ++i) {
                ki[i] = (i % 11 == 0) ? (int32_t)(i / k) : (int32_t)(rng() % (uint64_t)n);
                kd[i] = (float)(rng() % 4096) / 4096.0f;
            }
            int64_t a = 0, b = 0;
            CHECK(fdr_overlaps_write(whole.c_str(), 0, 1, n, 0, n, k, ki.data(), kd.data(), name_off.data(), names.data(),
                                     st, threads, &a) == 0);
            CHECK(fdr_overlaps_write_csr(parts.c_str(), 0, 1, n, 0, n, kp.data(), ki.data(), kd.data(), name_off.data(),
                                         names.data(), st, threads, &b) == 0);
            CHECK(a == b && slurp(whole) == slurp(parts));
            // refusals: nothing read out of bounds
            std::vector<int64_t> bad = indptr;
            if (n > 2) {
                bad[2] = bad[1] - 1 >= 0 ? bad[1] - 1 : bad[1];
                if (bad[2] < bad[1])
                    CHECK(fdr_overlaps_write_csr(parts.c_str(), 0, 1, n, 0, n, bad.data(), idx.data(), dist.data(),
                                                 name_off.data(), names.data(), st, threads, nullptr) == FDR_E_ARG);
            }
            CHECK(fdr_overlaps_write_csr(parts.c_str(), 0, 1, n, 0, n, nullptr, idx.data(), dist.data(), name_off.data(),
                                         names.data(), st, threads, nullptr) == FDR_E_ARG);
            CHECK(fdr_overlaps_write_csr(parts.c_str(), 0, 1, n, 1, n, indptr.data(), idx.data(), dist.data(),
                                         name_off.data(), names.data(), st, threads, nullptr) == FDR_E_ARG);
            std::vector<int32_t> out_of_range = idx;
            if (!out_of_range.empty()) {
                out_of_range[0] = (int32_t)n;
                CHECK(fdr_overlaps_write_csr(parts.c_str(), 0, 1, n, 0, n, indptr.data(), out_of_range.data(), dist.data(),
                                             name_off.data(), names.data(), st, threads, nullptr) == FDR_E_ARG);
            }
            ++cases;
        }
    // no rows at all
    {
        const int64_t name_off[3] = {0, 1, 2}, ip[1] = {0};
        const uint8_t st[2] = {0, 1};
        int64_t lines = -1;
        const std::string p = dir + "/empty.tsv";
        CHECK(fdr_overlaps_write_csr(p.c_str(), 0, 1, 2, 0, 0, ip, nullptr, nullptr, name_off, "ab", st, threads, &lines) == 0);
        CHECK(lines == 0 && slurp(p) == ovw::kHeader);
    }
    printf("rc=0 lines=%lld cases=%d\n", total_lines, cases);
    return 0;
}
