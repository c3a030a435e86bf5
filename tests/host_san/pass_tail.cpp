// Host-only build of the pass-tail schedule (live_issue_order, round_ready_points in knn_plan.inc) under
// AddressSanitizer + UBSan: tests/test_pass_tail_plan.py builds this with the flags of test_host_san.py and runs it.
//
//   pass_tail  -> random block masks, several segment counts, launch sizes and queue counts, with and without a
//                 minimum group size (groups that join the next larger NL); prints "rc=<0|1> plans=<n> joined=<n>
//                 early=<n> late_only=<n>" and a FAIL line per broken invariant
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
#include <thread>
#include <vector>

#include "../../include/fedrann_hip.h"
#include "../../fedrann_amd/csrc/host_common.inc"
#include "../../fedrann_amd/csrc/knn_plan.inc"

static int fail(const char *what, int nqb, int nseg, long long per, int queues, int trigger) {
    printf("FAIL %s nqb=%d nseg=%d per=%lld queues=%d trigger=%d\n", what, nqb, nseg, per, queues, trigger);
    return 1;
}

int main() {
    std::mt19937 rng(3601);
    long long plans = 0, joined = 0, early = 0, late_only = 0;
    for (int round = 0; round < 400; ++round) {
        const int nqb = 1 + (int)(rng() % 300), nseg = 1 + (int)(rng() % 6);
        const int shape = (int)(rng() % 4);  // 0: any mask, 1: only dense blocks, 2: no dense block, 3: two NL values
        std::vector<unsigned> masks((size_t)nqb);
        for (unsigned &m : masks) {
            m = rng() & 0xffu;
            if (shape == 1) m |= 0x7fu;
            if (shape == 2) m &= 0x3fu;
            if (shape == 3) m = (rng() & 1) ? 0x03u : 0x1fu;
        }
        const long long per = (round % 3 == 0) ? 0 : 1 + (long long)(rng() % 64);
        const LivePlan P = live_plan(masks.data(), nqb, nseg, (round & 1) ? per : 0);
        ++plans;
        {  // (a group that joined: some block runs on a larger instance than its own count asks for)
            bool any = false;
            for (const LiveGroup &g : P.groups)
                for (int i = 0; i < g.count && g.nl != FDR_LIVE_DENSE; ++i)
                    any |= std::max(live_popcount8(masks[(size_t)P.order[(size_t)(g.first + i)]]), FDR_LIVE_MIN_NL) < g.nl;
            joined += any;
        }
        const std::vector<int> asc = live_issue_order(P, false), desc = live_issue_order(P, true);
        if (asc.size() != P.groups.size() || desc.size() != P.groups.size()) return fail("order size", nqb, nseg, per, 0, 0);
        for (size_t i = 0; i < asc.size(); ++i) {
            if (asc[i] != (int)i || desc[i] != (int)(asc.size() - 1 - i)) return fail("order", nqb, nseg, per, 0, 0);
            if (i > 0 && P.groups[(size_t)desc[i]].nl >= P.groups[(size_t)desc[i - 1]].nl)
                return fail("descending nl", nqb, nseg, per, 0, 0);
        }
        if (!desc.empty() && P.groups.back().nl == FDR_LIVE_DENSE && desc[0] != (int)P.groups.size() - 1)
            return fail("dense first", nqb, nseg, per, 0, 0);
        std::vector<long long> items;
        for (int g : desc) items.push_back((long long)P.groups[(size_t)g].count * nseg);
        for (int queues = 1; queues <= 2; ++queues) {
            const std::vector<RoundLaunch> S = round_schedule(items, per, queues);
            for (int trigger = FDR_TAIL_TRIGGER_NONE; trigger <= FDR_TAIL_TRIGGER_GROUP; ++trigger) {
                const std::vector<int> at = round_ready_points(S, items.size(), queues, trigger);
                if (at.size() != items.size()) return fail("ready size", nqb, nseg, per, queues, trigger);
                bool any = false;
                for (size_t g = 0; g < at.size(); ++g) {
                    int last = -1;
                    for (size_t i = 0; i < S.size(); ++i)
                        if (S[i].group == (int)g) last = (int)i;
                    if (at[g] < 0) continue;
                    any = true;
                    // queued behind every launch of the group, in front of some launch, never for the last group
                    if (trigger == FDR_TAIL_TRIGGER_NONE || last < 0 || at[g] <= last || at[g] >= (int)S.size() ||
                        (int)g == S.back().group)
                        return fail("ready point", nqb, nseg, per, queues, trigger);
                    if (trigger == FDR_TAIL_TRIGGER_GROUP && at[g] != last + 1) return fail("group trigger", nqb, nseg, per, queues, trigger);
                    if (trigger == FDR_TAIL_TRIGGER_LAST && at[g] != (int)S.size() - std::min<int>(queues, (int)S.size()))
                        return fail("last trigger", nqb, nseg, per, queues, trigger);
                }
                if (trigger == FDR_TAIL_TRIGGER_GROUP)  // every group but the last is early
                    for (size_t g = 0; g < at.size(); ++g)
                        if ((at[g] < 0) != ((int)g == S.back().group)) return fail("group trigger covers", nqb, nseg, per, queues, trigger);
                if (items.size() == 1 && any) return fail("one group", nqb, nseg, per, queues, trigger);
                early += any;
                late_only += !any && trigger != FDR_TAIL_TRIGGER_NONE;
            }
        }
    }
    {  // by hand: groups of 5, 2 and 3 items in launches of 2 on two queues: launches g0 g0 g0 g1 g2 g2
        const std::vector<RoundLaunch> S = round_schedule({5, 2, 3}, 2, 2);
        const std::vector<int> a = round_ready_points(S, 3, 2, FDR_TAIL_TRIGGER_LAST);
        const std::vector<int> b = round_ready_points(S, 3, 2, FDR_TAIL_TRIGGER_GROUP);
        // LAST: the final launches are 4 and 5; groups 0 and 1 are complete in front of launch 4
        if (S.size() != 6 || a != std::vector<int>({4, 4, -1}) || b != std::vector<int>({3, 4, -1}))
            return fail("by hand", 0, 0, 2, 2, 0);
        // ... with one more item in group 1 its last launch is one of the final two: it stays behind the join
        const std::vector<RoundLaunch> T = round_schedule({4, 3, 1}, 2, 2);  // g0 g0 g1 g1 g2
        if (T.size() != 5 || round_ready_points(T, 3, 2, FDR_TAIL_TRIGGER_LAST) != std::vector<int>({3, -1, -1}))
            return fail("by hand 2", 0, 0, 2, 2, 0);
    }
    printf("rc=0 plans=%lld joined=%lld early=%lld late_only=%lld\n", plans, joined, early, late_only);
    return 0;
}
