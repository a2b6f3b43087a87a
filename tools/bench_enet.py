#!/usr/bin/env python3
"""Trial time of an elastic-net solve (l2 > 0: zf_trial_enet_kernel, F(x0) with the ridge term) beside its l1 sibling (l2 = 0:
the code of every earlier release) on the SAME device matrix, one JSON line per process.

    python tools/bench_enet.py --m 200000 --n 1000003 --per-col 8 --seed 7 --loss ls         # SparseLeastSquaresL1
    python tools/bench_enet.py --m 200000 --n 1000003 --per-col 8 --seed 7 --loss logistic   # SparseLogisticL1
    python tools/bench_enet.py --m 8192 --n 32768 --backend dense --loss ls --warmup 48      # LeastSquaresL1, A drawn in HBM

The protocol is tools/bench_logistic.py's (its builders and its timed_run are imported): the problem is seeded, built in this
process and lives in HBM before anything is timed; W untimed passes, a synchronise, K timed passes, a synchronise; FISTA from
lr = 1, one trial per pass.  The two problems - ``prob`` and ``prob.with_penalty(lam, l2)``, the same matrix handle -
ALTERNATE `repeats` times: l1, enet, l1, enet, ...  l2 = --l2-over-lam times lam (default 1).

The prox step of both moves the same 32 n bytes (x_k, x_{k-1}, grad in; x+ out) and the elastic-net body adds two VALU
operations per element, so the rule of DESIGN 4.5c applies: the medians may differ by at most the summed spread of the two
sets of repeats.  ``within_spread`` says whether they do; the difference is reported only when every timed trial of both was
accepted (a rejected trial is followed by one without the A^T sweep)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_logistic import build_dense, build_sparse, timed_run  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--backend", choices=("sparse", "dense"), default="sparse")
    ap.add_argument("--loss", choices=("ls", "logistic"), default="ls")
    ap.add_argument("--l2-over-lam", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    from zfista_amd.problems import LeastSquaresL1, LogisticL1, SparseLeastSquaresL1, SparseLogisticL1

    t0 = time.time()
    A, b_ls, lam_ls, labels, lam_lg = build_dense(args) if args.backend == "dense" else build_sparse(args)
    m, n = int(A.shape[0]), int(A.shape[1])
    sparse = args.backend == "sparse"
    if args.loss == "ls":
        lam = lam_ls
        base = SparseLeastSquaresL1(A, b_ls, lam) if sparse else LeastSquaresL1(A, b_ls, lam)
    else:
        lam = lam_lg
        base = SparseLogisticL1(A, labels, lam) if sparse else LogisticL1(A, labels, lam)
    l2 = args.l2_over_lam * lam
    probs = {"l1": base, "enet": base.with_penalty(lam, l2)}
    out = dict(tool="bench_enet", label=args.label, backend=args.backend, loss=args.loss, m=m, n=n, seed=args.seed, lam=lam, l2=l2,
               warmup=args.warmup, steps=args.steps, repeats=args.repeats, build_s=round(time.time() - t0, 2))
    if sparse:
        out["nnz"] = int(A.nnz)
    print(f"built {m} x {n} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    runs = {k: [] for k in probs}
    for _ in range(args.repeats):
        for k, prob in probs.items():   # alternated: l1, enet, l1, enet, ...
            runs[k].append(timed_run(prob, n, args.warmup, args.steps))
    for k, rs in runs.items():
        wall = [r["ms_per_trial_wall"] for r in rs]
        out[k] = dict(plan=rs[0]["plan"], ms_per_trial_wall=wall, ms_per_trial_wall_median=float(np.median(wall)),
                      ms_per_trial_wall_spread=float(max(wall) - min(wall)), ms_per_trial_events=[r["ms_per_trial_events"] for r in rs],
                      accepted=[r["accepted"] for r in rs], warmup_accepted=[r["warmup_accepted"] for r in rs], lr=rs[-1]["lr"])
    full = all(a == args.steps for k in runs for a in out[k]["accepted"])
    out["windows_all_accepted"] = full
    diff = out["enet"]["ms_per_trial_wall_median"] - out["l1"]["ms_per_trial_wall_median"]
    out["enet_minus_l1_ms_per_trial"] = diff if full else None
    out["summed_spread_ms"] = out["enet"]["ms_per_trial_wall_spread"] + out["l1"]["ms_per_trial_wall_spread"]
    out["within_spread"] = bool(diff <= out["summed_spread_ms"]) if full else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
