#!/usr/bin/env python3
"""Kernel durations per trial of the TIMED window of a solve, from a kernel trace of its own.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python3 tools/bench_logistic.py ... --loss logistic --repeats 1
    python3 tools/trace_trials.py DIR --trials 64 [--label NAME]

Reads DIR/**/*kernel_trace.csv and orders the launches by start time.  A solve that advances one trial per pass launches
the same kernels in the same order every trial (the guards are inside the kernels), and the timed passes are the last thing
the process launches: the last kernel that was launched more than `trials` times closes a trial, so the launches after
its (trials + 1)-th occurrence from the end, up to its last, are the window of the last `trials` trials.  Prints one JSON line: per kernel of the window its launches per trial,
the median and the mean duration of a launch and its microseconds per trial; their sum; and the window's wall time per
trial (first start to last end - the sum plus the gaps between the launches).  A launch that its guard ends at once (no
gradient due after a rejected trial) counts with the few microseconds it takes: means are over all launches of the window."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics


def short(name):
    return name.split("(")[0].replace("void ", "").strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--trials", type=int, default=64)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    rows = []
    for path in glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    if not rows:
        raise SystemExit(f"no *kernel_trace.csv under {args.dir}")
    rows.sort()
    count = {}
    for r in rows:
        count[r[2]] = count.get(r[2], 0) + 1
    closer = next((r[2] for r in reversed(rows) if count[r[2]] > args.trials), None)   # (a poll's or a flush's kernel may follow)
    if closer is None:
        raise SystemExit(f"no kernel was launched more than {args.trials} times: no window of {args.trials} trials")
    ends = [i for i, r in enumerate(rows) if r[2] == closer]
    window = rows[ends[-args.trials - 1] + 1:ends[-1] + 1]
    per = {}
    for s, e, name in window:
        per.setdefault(name, []).append((e - s) / 1e3)
    kernels = {name: dict(launches_per_trial=len(d) / args.trials, median_us=round(statistics.median(d), 3),
                          mean_us=round(sum(d) / len(d), 3), us_per_trial=round(sum(d) / args.trials, 3))
               for name, d in sorted(per.items(), key=lambda kv: -sum(kv[1]))}
    print(json.dumps(dict(tool="trace_trials", label=args.label, trials=args.trials, closing_kernel=closer,
                          launches_per_trial=len(window) / args.trials, kernels=kernels,
                          kernel_us_per_trial=round(sum(sum(d) for d in per.values()) / args.trials, 3),
                          window_us_per_trial=round((window[-1][1] - window[0][0]) / 1e3 / args.trials, 3))))


if __name__ == "__main__":
    main()
