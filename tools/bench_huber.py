#!/usr/bin/env python3
"""Rate of a device-resident Huber solve (HuberL1 / SparseHuberL1) beside its least-squares sibling on the SAME matrix and
right-hand side, one JSON line per process.

    python tools/bench_huber.py --m 200000 --n 1000003 --per-col 8 --seed 7                    # SparseHuberL1 | SparseLeastSquaresL1
    python tools/bench_huber.py --m 8192 --n 32768 --density 0.01                             # the same, uniform density
    python tools/bench_huber.py --m 16384 --n 65536 --backend dense --warmup 48 --repeats 3   # HuberL1 | LeastSquaresL1, A drawn in HBM
    python tools/bench_huber.py ... --loss huber --repeats 1                                  # one class alone (a profiler run:
                                                                                              #  tools/trace_trials.py reads its trace)

The protocol is tools/bench_logistic.py's (its builders and its timed window are imported): the problem is seeded, built in
this process and lives in HBM before anything is timed; W untimed passes, a synchronise, K timed passes of NativeRun.advance, a
synchronise; FISTA from lr = 1, one trial per pass.  --loss both (default) ALTERNATES the two classes `repeats` times in this
one process - ls, huber, ls, huber, ... - each run a fresh solver on the resident problem: the sibling's code is the
yardstick, and alternation keeps clocks and neighbours the same for both.  b is the least-squares right-hand side with an
outlier of +-5 std(b) on a seeded tenth of the rows (both classes get the same b), delta the median of |b|, lam a tenth of the
smallest that gives x = 0 for the class.

Reported per loss: ms per trial (wall) of every repeat with median and spread, accepted iterations per second, the solver's
own event time, the plan, the share of rows clipped at x = 0; the difference of the medians, only when every timed trial of
both classes was accepted (a rejected trial is followed by one without the A^T sweep: windows with rejections do not hold the
same work).  The rule of DESIGN 4.5c: a Huber trial may exceed a sibling trial by at most (Huber row kernels - residual
kernels, from one kernel trace per class) + the summed spread of the two sets of repeats.  The loss kernels move the bytes of
the residual kernels they replace (32 m at y, 16 m at x+)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_logistic import build_dense, build_sparse, timed_run  # noqa: E402
from tools.bench_sparse import PEAK_BYTES_PER_S, algorithmic_bytes, lengths  # noqa: E402


def add_outliers(b, seed):
    """b with +-5 std(b) added on a seeded tenth of its rows, and delta = median |b| (host array or CUDA tensor)."""
    rng = np.random.default_rng(seed + 1000)
    m = int(b.shape[0])
    rows = rng.choice(m, max(1, m // 10), replace=False)
    bump = rng.choice([-1.0, 1.0], rows.size)
    if isinstance(b, np.ndarray):
        out = b.copy()
        out[rows] += bump * 5.0 * float(np.std(b))
        return out, float(np.median(np.abs(out)))
    import torch

    out = b.clone()
    out[torch.from_numpy(rows).to(out.device)] += torch.from_numpy(bump).to(out.device) * 5.0 * float(out.std(unbiased=False))
    return out, float(out.abs().median())


def lam_tenth(A, cand):
    """0.1 |A^T cand|_inf: a tenth of the smallest lam that gives x = 0 (scale 1/2: grad f(0) = A^T cand up to its sign)."""
    if isinstance(cand, np.ndarray):
        return 0.1 * float(np.max(np.abs(A.T @ cand)))
    return 0.1 * float((A.T @ cand).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--backend", choices=("sparse", "dense"), default="sparse")
    ap.add_argument("--loss", choices=("both", "huber", "ls"), default="both")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    from zfista_amd.problems import HuberL1, LeastSquaresL1, SparseHuberL1, SparseLeastSquaresL1

    t0 = time.time()
    A, b_ls, _, _, _ = build_dense(args) if args.backend == "dense" else build_sparse(args)
    b, delta = add_outliers(b_ls, args.seed)
    clip = (lambda v: np.clip(v, -delta, delta)) if isinstance(b, np.ndarray) else (lambda v: v.clamp(-delta, delta))
    lam_ls, lam_hub = lam_tenth(A, b), lam_tenth(A, clip(b))
    m, n = int(A.shape[0]), int(A.shape[1])
    share0 = float((abs(b) > delta).sum()) / m
    out = dict(tool="bench_huber", label=args.label, backend=args.backend, loss=args.loss, m=m, n=n, seed=args.seed, warmup=args.warmup,
               steps=args.steps, repeats=args.repeats, delta=delta, clipped_share_at_0=share0, lam_ls=lam_ls, lam_huber=lam_hub,
               build_s=round(time.time() - t0, 2))
    sparse = args.backend == "sparse"
    if sparse:
        out.update(nnz=int(A.nnz), row_len_A=lengths(A.indptr), row_len_At=lengths(A.T.tocsr().indptr))
    print(f"built {m} x {n} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    probs = {}
    if args.loss in ("both", "ls"):
        probs["ls"] = SparseLeastSquaresL1(A, b, lam_ls) if sparse else LeastSquaresL1(A, b, lam_ls)
    if args.loss in ("both", "huber"):
        probs["huber"] = SparseHuberL1(A, b, lam_hub, delta) if sparse else HuberL1(A, b, lam_hub, delta)
    runs = {k: [] for k in probs}
    for _ in range(args.repeats):
        for k, prob in probs.items():   # alternated: ls, huber, ls, huber, ...
            runs[k].append(timed_run(prob, n, args.warmup, args.steps))
    for k, rs in runs.items():
        wall = [r["ms_per_trial_wall"] for r in rs]
        out[k] = dict(plan=rs[0]["plan"], ms_per_trial_wall=wall, ms_per_trial_wall_median=float(np.median(wall)),
                      ms_per_trial_wall_spread=float(max(wall) - min(wall)), ms_per_trial_events=[r["ms_per_trial_events"] for r in rs],
                      it_per_s=[r["it_per_s"] for r in rs], accepted=[r["accepted"] for r in rs],
                      warmup_accepted=[r["warmup_accepted"] for r in rs], lr=rs[-1]["lr"])
    if len(runs) == 2:
        full = all(a == args.steps for k in runs for a in out[k]["accepted"])
        out["windows_all_accepted"] = full
        out["huber_minus_ls_ms_per_trial"] = (out["huber"]["ms_per_trial_wall_median"] - out["ls"]["ms_per_trial_wall_median"]) if full else None
        out["summed_spread_ms"] = out["huber"]["ms_per_trial_wall_spread"] + out["ls"]["ms_per_trial_wall_spread"]
    if sparse:
        nbytes = algorithmic_bytes(m, n, int(A.nnz))
        out["algorithmic_bytes_per_trial"] = nbytes
        if "huber" in out:
            out["huber_fraction_of_8TBps"] = nbytes / (1e-3 * out["huber"]["ms_per_trial_wall_median"]) / PEAK_BYTES_PER_S
    else:
        out["dense_bytes_per_sweep"] = 8 * m * n
    print(json.dumps(out))


if __name__ == "__main__":
    main()
