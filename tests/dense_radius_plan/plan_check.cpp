// Host-only check of the dense radius search's target chunks (knn_plan.inc: radius_chunks / radius_chunk_rows) against
// the planner: for every index size given on the command line, every chunk's range plan must fit SegBounds
// (at most FDR_MAX_SEG segments), keep its segments within 2^FDR_PREFILTER_MAX_IB rows and cover the chunk, and the
// chunks must cover the index once.  Prints one line per size: n chunks chunk_rows max_nseg; exits 1 on a violation.
#include <algorithm>
#include <atomic>
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
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/fedrann_hip.h"
#include "../../fedrann_amd/csrc/host_common.inc"
#include "../../fedrann_amd/csrc/knn_plan.inc"

int main(int argc, char **argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        const int64_t n = atoll(argv[a]);
        const int64_t chunks = radius_chunks(n), len = radius_chunk_rows(n);
        int64_t covered = 0;
        int max_nseg = 0;
        for (int d : {128, 500}) {
            covered = 0;
            for (int64_t t0 = 0; t0 < n; t0 += len) {
                const int64_t rows = std::min<int64_t>(len, n - t0);
                if (rows > FDR_RADIUS_CHUNK_ROWS || (t0 % 32) != 0) ++bad;
                const int64_t nq = 65536;  // (a row block of the command line: the ping-pong shapes)
                const int shape = range_shape(padded_dim(d), (int)nq, (int)nq);
                const KnnPlan p = knn_plan(256, nq, rows, d, 1, shape);
                if (p.nseg < 1 || p.nseg > FDR_MAX_SEG || p.segs.b[0] != 0 || p.segs.b[p.nseg] < rows) ++bad;
                for (int s = 0; s < p.nseg && s < FDR_MAX_SEG; ++s)
                    if (p.segs.b[s + 1] <= p.segs.b[s] || p.segs.b[s + 1] - p.segs.b[s] > (1 << FDR_PREFILTER_MAX_IB)) ++bad;
                max_nseg = std::max(max_nseg, p.nseg);
                covered += rows;
            }
            if (covered != n) ++bad;
        }
        printf("%lld %lld %lld %d\n", (long long)n, (long long)chunks, (long long)len, max_nseg);
    }
    return bad ? 1 : 0;
}
