#!/usr/bin/env python
"""The end of the candidate pass in a rocprofv3 --kernel-trace run of bench.py (docs/experiments.md A-36).

usage: python devtools/pass_tail.py <dir with *kernel_trace.csv> [out.json]

A step begins at its live_block_masks_kernel dispatch (once per prefilter call).  Per step, from the dispatches' begin and
end timestamps: the ends of the last and the second-to-last candidate-pass dispatch, the start of the first and of the
last knn_merge_keys_kernel, how many merge / re-rank dispatches begin before the pass ends, and the duration of the last
pass dispatches on each queue against the median of their instance's full launches.  Prints the median over the steps.
"""
import csv
import glob
import json
import os
import re
import statistics
import sys


def load(path):
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % path)
    rows = []
    for r in csv.DictReader(open(files[0])):
        grid = int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)
        wg = int(r.get("Workgroup_Size", r.get("Workgroup_Size_X", 1)) or 1)
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], grid // max(wg, 1),
                     r.get("Queue_Id", "")))
    rows.sort()
    return rows


def instance(name):
    m = re.search(r"knn_prefilter_live_kernel(?:<|ILi)(\d+)", name)  # (demangled or mangled)
    if m:
        return "live%s" % m.group(1)
    return "dense" if "knn_prefilter" in name else None


def main():
    rows = load(sys.argv[1])
    starts = [i for i, r in enumerate(rows) if "live_block_masks_kernel" in r[2]]
    steps = []
    for a, b in zip(starts, starts[1:] + [len(rows)]):
        step = rows[a:b]
        pas = [r for r in step if instance(r[2])]
        mk = [r for r in step if "knn_merge_keys_kernel" in r[2]]
        rr = [r for r in step if "knn_rerank_kernel" in r[2]]
        if len(pas) < 3 or not mk or not rr:
            continue
        by_end = sorted(pas, key=lambda r: r[1])
        last, second = by_end[-1], by_end[-2]
        full = {}
        for r in pas:
            full.setdefault((instance(r[2]), r[3]), []).append(r[1] - r[0])
        steady = {k: statistics.median(v) for k, v in full.items()}

        def rel(r):  # a final dispatch against the median of its instance's launches of the same size
            return {"instance": instance(r[2]), "workgroups": r[3], "ms": (r[1] - r[0]) / 1e6,
                    "steady_ms": steady[(instance(r[2]), r[3])] / 1e6, "same_size_launches": len(full[(instance(r[2]), r[3])])}
        t0 = min(r[0] for r in pas)
        steps.append({
            "pass_ms": (last[1] - t0) / 1e6,
            "pass_dispatches": len(pas),
            "order": [k for k, _ in sorted(((instance(r[2]), r[0]) for r in pas), key=lambda x: x[1])],
            "second_to_last_end_before_last_end_ms": (last[1] - second[1]) / 1e6,
            "last": rel(last), "second_to_last": rel(second),
            "first_merge_start_after_pass_end_ms": (mk[0][0] - last[1]) / 1e6,
            "last_merge_start_after_pass_end_ms": (mk[-1][0] - last[1]) / 1e6,
            "last_rerank_end_after_pass_end_ms": (max(r[1] for r in rr) - last[1]) / 1e6,
            "merge_dispatches": len(mk), "rerank_dispatches": len(rr),
            "merge_rerank_started_before_pass_end": sum(1 for r in mk + rr if r[0] < last[1]),
            "merge_ms": sum(r[1] - r[0] for r in mk) / 1e6, "rerank_ms": sum(r[1] - r[0] for r in rr) / 1e6,
            # (name, workgroups, begin, end) in ms from the pass's first dispatch
            "timeline": [[instance(r[2]) or ("merge" if "merge" in r[2] else "rerank"), r[3],
                          round((r[0] - t0) / 1e6, 4), round((r[1] - t0) / 1e6, 4)] for r in sorted(pas + mk + rr)],
        })
    if not steps:
        sys.exit("no step with a live-chunk pass in the trace")
    for s in steps:  # the groups in issue order, once each
        seen = []
        for k in s["order"]:
            if not seen or seen[-1] != k:
                seen.append(k)
        s["order"] = seen

    def med(get):
        return round(statistics.median(get(s) for s in steps), 4)
    keys = [k for k, v in steps[0].items() if isinstance(v, (int, float))]
    out = {"steps": len(steps), "group_order": steps[-1]["order"], "median": {k: med(lambda s, k=k: s[k]) for k in keys}}
    for which in ("last", "second_to_last"):
        out["median"][which] = {"instance": steps[-1][which]["instance"], "workgroups": steps[-1][which]["workgroups"],
                                "ms": med(lambda s: s[which]["ms"]), "steady_ms": med(lambda s: s[which]["steady_ms"]),
                                "same_size_launches": steps[-1][which]["same_size_launches"]}
    out["last_step"] = steps[-1]
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text + "\n")


if __name__ == "__main__":
    main()
