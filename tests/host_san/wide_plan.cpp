// Host-only build of the k-NN launch planner (knn_plan.inc) under AddressSanitizer + UBSan, for the calls beyond
// k <= 64: tests/test_wide_plan.py builds this with the flags of test_host_san.py and runs it.
//
//   wide_plan   -> sweeps knn_route / knn_plan over dp, k, target and query counts and CU counts; prints
//                  "rc=<0|1> plans=<n> wide=<n> generic=<n>" and a FAIL line per broken invariant
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "../../include/fedrann_hip.h"
#include "../../fedrann_amd/csrc/host_common.inc"
#include "../../fedrann_amd/csrc/knn_plan.inc"

static int fail(const char *what, int cus, int64_t nq, int64_t nt, int dp, int k) {
    printf("FAIL %s cus=%d nq=%lld nt=%lld dp=%d k=%d\n", what, cus, (long long)nq, (long long)nt, dp, k);
    return 1;
}

// the exact plan of a FDR_ROUTE_WIDE call: a release tile kernel of its dp (dp = 1024: the split-K family) with at most
// 128 queries per workgroup, at least one workgroup per CU in 160 KiB of LDS, well-formed segments, no more keys per
// query than the k > 64 merge stages, and the partial lists the workspace holds
static int check_wide(int cus, int64_t nq, int64_t nt, int dp, int k) {
    const KnnPlan p = knn_plan(cus, nq, nt, dp, k);
    const KnnShape &sh = kShapes[p.shape];
    const int family = dp == 1024 ? FDR_FAM_TILE_SPLIT : FDR_FAM_TILE;
    if (!(sh.family == family && sh.release && sh.dp == dp && sh.qw() <= 128))
        return fail("shape", cus, nq, nt, dp, k);
    if (!(knn_lds_bytes(sh, k) <= 160 * 1024 && knn_wg_per_cu(sh, k) >= 1)) return fail("lds", cus, nq, nt, dp, k);
    const int T = (int)((nt + 31) / 32);
    bool ok = p.nseg >= 1 && p.nseg <= FDR_MAX_SEG && p.segs.b[0] == 0 && p.qw == sh.qw() &&
              (int64_t)p.nqb * p.qw >= nq && p.nq_pad == p.nqb * p.qw && p.cohort == 0 && p.queues == 1;
    for (int i = 0; i < p.nseg && ok; ++i) {
        const int len = p.segs.b[i + 1] - p.segs.b[i];
        ok = len > 0 && len % 32 == 0;
    }
    ok = ok && p.segs.b[p.nseg] == T * 32;
    for (int i = p.nseg; i <= FDR_MAX_SEG && ok; ++i) ok = p.segs.b[i] == T * 32;
    if (!ok) return fail("segments", cus, nq, nt, dp, k);
    if (k > FDR_FAST_MAX_K && p.nseg * k > FDR_MERGE_WIDE_CAP) return fail("merge", cus, nq, nt, dp, k);
    if (!(p.partial_bytes == (size_t)p.nseg * p.nq_pad * (size_t)k * 8 &&
          p.total_bytes == p.bits_bytes + p.shared_bytes + p.partial_bytes))
        return fail("workspace", cus, nq, nt, dp, k);
    return 0;
}

int main() {
    int bad = 0, plans = 0, wide = 0, generic = 0;
    const int64_t sizes[] = {20, 129, 8191, 8192, 8193, (1 << 19) - 1, 1 << 19, 1000000, 10000000};
    for (int cus : {64, 256, 304})
        for (int64_t nt : sizes)
            for (int dp : {128, 256, 512, 1024, 2048})
                for (int k : {1, 20, 64, 65, 100, 128}) {
                    if (nt < k) continue;
                    const int route = knn_route(dp, k, nt);
                    const int want = dp <= 512 && k <= 64      ? FDR_ROUTE_FAST
                                     : dp <= 1024 && nt >= 8192 ? FDR_ROUTE_WIDE
                                                                : FDR_ROUTE_GENERIC;
                    if (route != want) bad += fail("route", cus, 0, nt, dp, k);
                    if (route == FDR_ROUTE_GENERIC) ++generic;
                    if (route != FDR_ROUTE_WIDE) continue;
                    ++wide;
                    for (int64_t nq : {nt, (nt + 7) / 8, (nt + 2) / 3, (int64_t)1}) {
                        if (nt >= 10000000 && nq > nt / 8) continue;  // (a rank's share: the planner's run time)
                        bad += check_wide(cus, nq, nt, dp, k);
                        ++plans;
                    }
                }
    printf("rc=%d plans=%d wide=%d generic=%d\n", bad ? 1 : 0, plans, wide, generic);
    return bad ? 1 : 0;
}
