#!/usr/bin/env python3
"""Rate of a device-resident solve with per-row sample weights (w = 1) beside its unweighted sibling on the SAME matrix and
right-hand side, one JSON line per process.

    python tools/bench_weights.py --m 200000 --n 1000003 --per-col 8 --seed 7                    # sparse, least squares
    python tools/bench_weights.py --m 16384 --n 65536 --backend dense --warmup 48 --repeats 5   # dense, A drawn in HBM
    python tools/bench_weights.py ... --loss logistic | huber                                   # the other two losses
    python tools/bench_weights.py ... --which weighted --repeats 1                              # one side alone (a profiler run)

The protocol is tools/bench_huber.py's (its builders and the timed window of tools/bench_logistic.py are imported): the problem
is seeded, built in this process and lives in HBM before anything is timed; W untimed passes, a synchronise, K timed passes of
NativeRun.advance, a synchronise; FISTA from lr = 1, one trial per pass.  The two sides are ALTERNATED `repeats` times in this
one process - plain, weighted, plain, weighted, ... - each run a fresh solver on the resident problem; the weighted side is
`problem.with_sample_weight(ones)`: the same matrix, b and handle, only w uploaded.  The yardstick is the unweighted sibling in
the same session, never the weighted code itself.

With w = 1 the logistic and Huber solves are bit-identical to their siblings (tests/test_gpu_weights.py), the least-squares
solve equal to rounding: both windows hold the same trials.  Reported per side: ms per trial (wall) of every repeat with median
and spread, accepted iterations per second, the solver's own event time, the plan; the difference of the medians when every
timed trial of both sides was accepted; `byte_share` = the 16 m bytes the weighted loss kernels read beyond their siblings per
accepted trial (8 m at y, 8 m at x+; csrc/zf_kernels_loss.h) over the algorithmic bytes of a trial.  The rule of DESIGN 4.5h:
a weighted trial may exceed a sibling trial by that share of the sibling's time plus the summed spread of the two sets of
repeats; beyond it, the kernel-trace durations of the loss kernels say where the time went."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_huber import add_outliers, lam_tenth  # noqa: E402
from tools.bench_logistic import build_dense, build_sparse, timed_run  # noqa: E402
from tools.bench_sparse import algorithmic_bytes, lengths  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--backend", choices=("sparse", "dense"), default="sparse")
    ap.add_argument("--loss", choices=("ls", "logistic", "huber"), default="ls")
    ap.add_argument("--which", choices=("both", "plain", "weighted"), default="both")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch

    from zfista_amd.problems import HuberL1, LeastSquaresL1, LogisticL1, SparseHuberL1, SparseLeastSquaresL1, SparseLogisticL1

    t0 = time.time()
    A, b_ls, lam_ls, labels, lam_lg = build_dense(args) if args.backend == "dense" else build_sparse(args)
    m, n = int(A.shape[0]), int(A.shape[1])
    sparse = args.backend == "sparse"
    if args.loss == "logistic":
        plain = SparseLogisticL1(A, labels, lam_lg) if sparse else LogisticL1(A, labels, lam_lg)
    elif args.loss == "huber":
        b, delta = add_outliers(b_ls, args.seed)
        clip = (lambda v: np.clip(v, -delta, delta)) if isinstance(b, np.ndarray) else (lambda v: v.clamp(-delta, delta))
        lam = lam_tenth(A, clip(b))
        plain = SparseHuberL1(A, b, lam, delta) if sparse else HuberL1(A, b, lam, delta)
    else:
        plain = SparseLeastSquaresL1(A, b_ls, lam_ls) if sparse else LeastSquaresL1(A, b_ls, lam_ls)
    weighted = plain.with_sample_weight(torch.ones(m, dtype=torch.float64, device="cuda"))
    shared = (weighted._spmat is plain._spmat) if sparse else (weighted.A.data_ptr() == plain.A.data_ptr())
    out = dict(tool="bench_weights", label=args.label, backend=args.backend, loss=args.loss, which=args.which, m=m, n=n, seed=args.seed,
               warmup=args.warmup, steps=args.steps, repeats=args.repeats, matrix_shared=bool(shared), build_s=round(time.time() - t0, 2))
    if sparse:
        out.update(nnz=int(A.nnz), row_len_A=lengths(A.indptr), row_len_At=lengths(A.T.tocsr().indptr))
    print(f"built {m} x {n} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    probs = {k: p for k, p in (("plain", plain), ("weighted", weighted)) if args.which in ("both", k)}
    runs = {k: [] for k in probs}
    for _ in range(args.repeats):
        for k, prob in probs.items():   # alternated: plain, weighted, plain, weighted, ...
            runs[k].append(timed_run(prob, n, args.warmup, args.steps))
    for k, rs in runs.items():
        wall = [r["ms_per_trial_wall"] for r in rs]
        out[k] = dict(plan=rs[0]["plan"], ms_per_trial_wall=wall, ms_per_trial_wall_median=float(np.median(wall)),
                      ms_per_trial_wall_spread=float(max(wall) - min(wall)), ms_per_trial_events=[r["ms_per_trial_events"] for r in rs],
                      it_per_s=[r["it_per_s"] for r in rs], accepted=[r["accepted"] for r in rs],
                      warmup_accepted=[r["warmup_accepted"] for r in rs], lr=rs[-1]["lr"])
    nbytes = algorithmic_bytes(m, n, int(A.nnz)) if sparse else 2 * 8 * m * n
    out["algorithmic_bytes_per_trial"] = nbytes
    out["extra_bytes_per_trial"] = 16 * m
    out["byte_share"] = 16 * m / nbytes
    if len(runs) == 2:
        full = all(a == args.steps for k in runs for a in out[k]["accepted"])
        pm, wm = out["plain"]["ms_per_trial_wall_median"], out["weighted"]["ms_per_trial_wall_median"]
        out["windows_all_accepted"] = full
        out["weighted_minus_plain_ms_per_trial"] = (wm - pm) if full else None
        out["weighted_over_plain"] = (wm / pm) if full else None
        out["summed_spread_ms"] = out["plain"]["ms_per_trial_wall_spread"] + out["weighted"]["ms_per_trial_wall_spread"]
        out["allowance_ms"] = out["byte_share"] * pm + out["summed_spread_ms"]
        out["within_allowance"] = (wm - pm <= out["allowance_ms"]) if full else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
