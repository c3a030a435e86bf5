// Host-only build of the live-chunk grouping (live_plan in knn_plan.inc) under AddressSanitizer + UBSan:
// tests/test_live_groups.py builds this with the flags of test_host_san.py and runs it.
//
//   live_groups  -> random and hand-made block masks, several segment counts and launch sizes; for every plan, and for
//                   a single group of all its blocks, the launches round_schedule deals (launch sizes 0, 1, 64, 512 on
//                   1, 2 and 4 queues); prints "rc=<0|1> plans=<n> merged=<n> schedules=<n>" and a FAIL line per
//                   broken invariant
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

static int fail(const char *what, int nqb, int nseg, long long min_items) {
    printf("FAIL %s nqb=%d nseg=%d min_items=%lld\n", what, nqb, nseg, min_items);
    return 1;
}

static int nl_of(unsigned m) {  // the instance a block would take by itself
    const int pc = live_popcount8(m);
    return pc > FDR_LIVE_MAX_NL ? FDR_LIVE_DENSE : std::max(pc, FDR_LIVE_MIN_NL);
}

// round_schedule over groups of `items`: every group's items [0, n) exactly once by launches with ascending, contiguous
// base; groups in the given order; no launch above the launch size and only a group's last one short; launch i on queue
// i % queues; launch size 0: exactly one launch per non-empty group
static int g_schedules;
static int check_schedule(const std::vector<long long> &items, int nqb, int nseg) {
    for (long long per : {0ll, 1ll, 64ll, 512ll})
        for (int queues : {1, 2, 4}) {
            const std::vector<RoundLaunch> S = round_schedule(items, per, queues);
            ++g_schedules;
            size_t i = 0;
            for (size_t g = 0; g < items.size(); ++g) {
                long long at = 0;
                int launches = 0;
                while (i < S.size() && S[i].group == (int)g) {
                    const RoundLaunch &l = S[i];
                    if (l.base != at || l.grid <= 0) return fail("schedule cover", nqb, nseg, per);
                    if (l.queue != (int)(i % (size_t)queues)) return fail("schedule queue", nqb, nseg, per);
                    if (per > 0 && l.grid > per) return fail("schedule launch size", nqb, nseg, per);
                    at += l.grid;
                    if (per > 0 && l.grid < per && at != items[g]) return fail("schedule short launch", nqb, nseg, per);
                    ++launches;
                    ++i;
                }
                if (at != items[g]) return fail("schedule group", nqb, nseg, per);  // (also: a group out of order)
                if (per == 0 && launches != (items[g] > 0 ? 1 : 0)) return fail("schedule one launch", nqb, nseg, per);
            }
            if (i != S.size()) return fail("schedule order", nqb, nseg, per);
        }
    return 0;
}

static int check(const std::vector<unsigned> &masks, int nseg, long long min_items, int &merged) {
    const int nqb = (int)masks.size();
    const LivePlan P = live_plan(masks.data(), nqb, nseg, min_items);
    {  // the launches of this plan's groups, and of a plain pass over the same blocks
        std::vector<long long> items;
        for (const LiveGroup &g : P.groups) items.push_back((long long)g.count * nseg);
        if (check_schedule(items, nqb, nseg) || check_schedule({(long long)nqb * nseg}, nqb, nseg)) return 1;
    }
    // every block exactly once; the groups tile `order`, ascending nl, blocks ascending inside a group (so that the work
    // items (segment, block of the group) are segment-major over an ascending block list)
    if ((int)P.order.size() != nqb || (int)P.ids.size() != nqb) return fail("sizes", nqb, nseg, min_items);
    std::vector<int> seen((size_t)nqb, 0);
    for (int b : P.order) {
        if (b < 0 || b >= nqb || seen[(size_t)b]++) return fail("once", nqb, nseg, min_items);
    }
    int at = 0, last_nl = 0;
    std::vector<int> group_of((size_t)nqb, 0);
    for (const LiveGroup &g : P.groups) {
        if (g.first != at || g.count <= 0 || g.nl <= last_nl) return fail("tiling", nqb, nseg, min_items);
        if (g.nl != FDR_LIVE_DENSE && (g.nl < FDR_LIVE_MIN_NL || g.nl > FDR_LIVE_MAX_NL)) return fail("nl", nqb, nseg, min_items);
        for (int i = 0; i < g.count; ++i) {
            const int b = P.order[(size_t)(g.first + i)];
            if (i > 0 && b <= P.order[(size_t)(g.first + i - 1)]) return fail("ascending", nqb, nseg, min_items);
            group_of[(size_t)b] = g.nl;
        }
        at += g.count;
        last_nl = g.nl;
    }
    if (at != nqb) return fail("cover", nqb, nseg, min_items);
    // a live group below one launch exists only if nothing larger could take it ... it always can (the dense kernel):
    // no live group is smaller than min_items; a block only ever moves UP; without merging it stays where it belongs
    for (const LiveGroup &g : P.groups)
        if (g.nl != FDR_LIVE_DENSE && (long long)g.count * nseg < min_items) return fail("small group", nqb, nseg, min_items);
    long long own[FDR_LIVE_DENSE + 1] = {};
    for (int b = 0; b < nqb; ++b) own[nl_of(masks[(size_t)b])]++;
    for (int b = 0; b < nqb; ++b) {
        const int want = nl_of(masks[(size_t)b]), got = group_of[(size_t)b];
        if (got < want) return fail("moved down", nqb, nseg, min_items);
        if (got != want) {
            ++merged;
            // moved up: only out of a group that (with what had moved into it) was below one launch
            if (min_items <= 0) return fail("moved without merging", nqb, nseg, min_items);
        }
        // the dense group holds exactly the blocks of seven or eight live chunks, unless the last live group joined it
        if (got == FDR_LIVE_DENSE && want != FDR_LIVE_DENSE) {
            long long below = 0;
            for (int nl = FDR_LIVE_MIN_NL; nl <= FDR_LIVE_MAX_NL; ++nl) below += own[nl];
            if (below * nseg >= min_items * (FDR_LIVE_MAX_NL - FDR_LIVE_MIN_NL + 1)) return fail("dense", nqb, nseg, min_items);
        }
        // ids: the group's nl chunk ids, ascending, a superset of the block's mask
        if (got != FDR_LIVE_DENSE) {
            unsigned m = 0;
            int prev = -1;
            for (int i = 0; i < got; ++i) {
                const int c = (int)((P.ids[(size_t)b] >> (4 * i)) & 15u);
                if (c <= prev || c > 7) return fail("ids order", nqb, nseg, min_items);
                prev = c;
                m |= 1u << c;
            }
            if ((m & masks[(size_t)b]) != (masks[(size_t)b] & 0xffu) || (P.ids[(size_t)b] >> (4 * got)) != 0u)
                return fail("ids cover", nqb, nseg, min_items);
        }
    }
    return 0;
}

int main() {
    int bad = 0, plans = 0, merged = 0;
    std::mt19937 rng(2207);
    for (int nqb : {1, 2, 7, 48, 391, 3247})
        for (int nseg : {1, 2, 5})
            for (long long min_items : {0ll, 1ll, 64ll, 512ll}) {
                for (int kind = 0; kind < 4; ++kind) {
                    std::vector<unsigned> masks((size_t)nqb);
                    for (int b = 0; b < nqb; ++b) {
                        unsigned m = 0;
                        const int want = kind == 0 ? (int)(rng() % 9) : kind == 1 ? 4 : kind == 2 ? 7 + (b & 1) : (b * 9) / nqb;
                        while (live_popcount8(m) < want) m |= 1u << (rng() % 8);
                        masks[(size_t)b] = m;
                    }
                    bad += check(masks, nseg, min_items, merged);
                    ++plans;
                }
            }
    // by hand: four blocks of NL 2 (one launch of 4 items at nseg = 1 holds them), one of NL 3 joins NL 4, dense stays dense
    {
        const std::vector<unsigned> masks = {0x03, 0x81, 0x00, 0x10, 0x07, 0x0f, 0x1e, 0x33, 0x3c, 0x7f, 0xff};
        const LivePlan P = live_plan(masks.data(), (int)masks.size(), 1, 4);
        const bool ok = P.groups.size() == 3 && P.groups[0].nl == 2 && P.groups[0].count == 4 && P.groups[1].nl == 4 &&
                        P.groups[1].count == 5 && P.groups[2].nl == FDR_LIVE_DENSE && P.groups[2].count == 2 &&
                        P.order == std::vector<int>({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}) && P.ids[2] == 0x10u &&
                        P.ids[3] == 0x40u && P.ids[4] == 0x3210u && P.ids[1] == 0x70u;
        if (!ok) bad += fail("by hand", (int)masks.size(), 1, 4);
        bad += check(masks, 1, 4, merged);
        ++plans;
    }
    // by hand: groups of 5, 0 and 3 items in launches of 2 on two queues -- the empty group launches nothing, and the deal
    // goes on across the groups
    {
        const std::vector<RoundLaunch> S = round_schedule({5, 0, 3}, 2, 2);
        const int want[5][4] = {{0, 0, 0, 2}, {0, 1, 2, 2}, {0, 0, 4, 1}, {2, 1, 0, 2}, {2, 0, 2, 1}};  // group, queue, base, grid
        bool ok = S.size() == 5;
        for (size_t i = 0; ok && i < 5; ++i)
            ok = S[i].group == want[i][0] && S[i].queue == want[i][1] && S[i].base == want[i][2] && S[i].grid == want[i][3];
        if (!ok) bad += fail("schedule by hand", 0, 1, 2);
        bad += check_schedule({5, 0, 3}, 0, 1) + check_schedule({}, 0, 1);
    }
    printf("rc=%d plans=%d merged=%d schedules=%d\n", bad ? 1 : 0, plans, merged, g_schedules);
    return bad ? 1 : 0;
}
