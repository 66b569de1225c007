"""Gaps around the giant stage's launch from a rocprofv3 --kernel-trace CSV.

    python profiles/inflight_tail/trace_gaps.py <dir with *kernel_trace.csv> [--last N] [--skip-last M]

Per hardware queue the dispatches are put in start order; for each
giant_search dispatch: the gap from the end of the memo_search before it to
its start, its duration, and the gap from its end to the start of the same
queue's next compact_search.  The calls taken are the last N giant_search
dispatches by start time (after dropping the last M), i.e. the timed window
of `bench.py --steps N`, or the roofline leg of `bench.py --full`.  Prints
one JSON line: median and p90 of each figure in microseconds.
"""
import argparse
import csv
import glob
import json
import os
import statistics


def rows(d):
    out = []
    for p in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        with open(p, newline="") as f:
            out.extend(csv.DictReader(f))
    return out


def kind(name):
    for k in ("giant_search", "memo_search", "compact_search"):
        if k in name:
            return k
    return None


def stat(v):
    if not v:
        return None
    v = sorted(v)
    return {"n": len(v), "median_us": round(statistics.median(v) / 1e3, 2),
            "p90_us": round(v[min(len(v) - 1, int(0.9 * len(v)))] / 1e3, 2),
            "min_us": round(v[0] / 1e3, 2), "max_us": round(v[-1] / 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--last", type=int, default=20)
    ap.add_argument("--skip-last", type=int, default=0)
    args = ap.parse_args()
    per_q = {}
    for r in rows(args.dir):
        k = kind(r["Kernel_Name"])
        if k:
            per_q.setdefault(r.get("Queue_Id", "0"), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k))
    calls = []           # (giant start, memo->giant gap, giant duration, giant->compact gap, compact duration)
    for q in per_q.values():
        q.sort()
        for i, (s, e, k) in enumerate(q):
            if k != "giant_search":
                continue
            before = q[i - 1] if i > 0 and q[i - 1][2] == "memo_search" else None
            after = q[i + 1] if i + 1 < len(q) and q[i + 1][2] == "compact_search" else None
            calls.append((s, s - before[1] if before else None, e - s, after[0] - e if after else None,
                          after[1] - after[0] if after else None))
    calls.sort()
    if args.skip_last:
        calls = calls[:-args.skip_last]
    calls = calls[-args.last:]
    print(json.dumps({"queues": len(per_q), "calls": len(calls),
                      "memo_end_to_giant_start": stat([c[1] for c in calls if c[1] is not None]),
                      "giant_duration": stat([c[2] for c in calls]),
                      "giant_end_to_next_compact_start": stat([c[3] for c in calls if c[3] is not None]),
                      "next_compact_duration": stat([c[4] for c in calls if c[4] is not None])}))


if __name__ == "__main__":
    main()
