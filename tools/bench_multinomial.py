#!/usr/bin/env python3
"""Rate of a device-resident multinomial solve (MultinomialL1 / SparseMultinomialL1) beside its one-vs-rest sibling
(MultiResponseLogisticL1 / SparseMultiResponseLogisticL1) on the SAME matrix and the same K, for K in {2, 4, 8, 16}: one JSON line
per process.

    python tools/bench_multinomial.py --m 200000 --n 1000003 --per-col 8 --seed 7          # the sparse classes
    python tools/bench_multinomial.py --m 16384 --n 65536 --backend dense --repeats 3      # the dense classes, A drawn in HBM
    python tools/bench_multinomial.py ... --K 8 --loss multinomial --repeats 1             # one class and one K alone (a profiler run)

The protocol is tools/bench_poisson.py's (the builders and the timed window of tools/bench_logistic.py are imported): the matrix is
seeded, built in this process and lives in HBM before anything is timed; W untimed passes, a synchronise, S timed passes of
NativeRun.advance, a synchronise; FISTA from lr = 1, one trial per pass.  For every K the two classes are ALTERNATED `repeats` times -
logistic, multinomial, logistic, multinomial, ... - each run a fresh solver on the resident problem.  Both losses are means over
the rows (scale = 1 / m), lam is a tenth of the smallest that gives x = 0 for the class.  The class labels are the argmax of
A X_true + Gumbel noise (a draw from the softmax model); the sibling's B is +1 on the label's column and -1 elsewhere.

The sibling runs the same two sweeps on the same bytes, so the difference of the medians is the row kernels': K exps, one log and
one division per row of K margins beside K exps, K log1ps and K divisions.  It is reported per K only when every timed trial of both
classes was accepted (a rejected trial is followed by one without the A^T sweep: windows with rejections do not hold the same work)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_logistic import build_dense, build_sparse, timed_run  # noqa: E402


def draw_labels(A, n, K, seed):
    """m class labels in 0 .. K-1: the argmax of A X_true + Gumbel noise, X_true with 200 non-zero rows (host int64 array)."""
    rng = np.random.default_rng(seed + 4000 + K)
    X = np.zeros((n, K))
    rows = rng.choice(n, min(200, n), replace=False)
    X[rows] = rng.standard_normal((rows.size, K))
    if isinstance(A, np.ndarray) or hasattr(A, "tocsr"):
        Z = np.asarray(A @ X)
    else:
        import torch

        Z = (A @ torch.from_numpy(X).to(A.device)).cpu().numpy()
    return np.argmax(Z + rng.gumbel(size=Z.shape), axis=1)


def lam_tenth(A, R, scale):
    """0.1 scale |A^T R|_inf for an (m, K) host array R."""
    if isinstance(A, np.ndarray) or hasattr(A, "tocsr"):
        return 0.1 * scale * float(np.max(np.abs(A.T @ R)))
    import torch

    return 0.1 * scale * float((A.T @ torch.from_numpy(R).to(A.device)).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--backend", choices=("sparse", "dense"), default="sparse")
    ap.add_argument("--loss", choices=("both", "multinomial", "logistic"), default="both")
    ap.add_argument("--K", type=int, nargs="*", default=[2, 4, 8, 16])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    from zfista_amd import problems as Z

    t0 = time.time()
    sparse = args.backend == "sparse"
    A = (build_sparse(args) if sparse else build_dense(args))[0]
    m, n = int(A.shape[0]), int(A.shape[1])
    scale = 1.0 / m
    out = dict(tool="bench_multinomial", label=args.label, backend=args.backend, loss=args.loss, m=m, n=n, seed=args.seed,
               warmup=args.warmup, steps=args.steps, repeats=args.repeats, scale=scale, build_s=round(time.time() - t0, 2), K={})
    if sparse:
        out["nnz"] = int(A.nnz)
    print(f"built {m} x {n} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    plain = (Z.SparseLogisticL1(A, np.ones(m), 1.0, scale=scale) if sparse else Z.LogisticL1(A, np.ones(m), 1.0, scale=scale))   # holds the matrix
    for K in args.K:
        lab = draw_labels(A, n, K, args.seed)
        Y = np.zeros((m, K))
        Y[np.arange(m), lab] = 1.0
        B = 2.0 * Y - 1.0
        probs = {}
        if args.loss in ("both", "logistic"):
            probs["logistic"] = plain.with_responses(B).with_lam(lam_tenth(A, B / 2, scale))
        if args.loss in ("both", "multinomial"):
            probs["multinomial"] = plain.with_classes(lab, n_classes=K).with_lam(lam_tenth(A, 1.0 / K - Y, scale))
        runs = {k: [] for k in probs}
        for _ in range(args.repeats):
            for k, prob in probs.items():   # alternated: logistic, multinomial, logistic, multinomial, ...
                runs[k].append(timed_run(prob, n * K, args.warmup, args.steps))
        rec = {}
        for k, rs in runs.items():
            wall = [r["ms_per_trial_wall"] for r in rs]
            rec[k] = dict(plan=rs[0]["plan"], lam=probs[k].lam, ms_per_trial_wall=wall, ms_per_trial_wall_median=float(np.median(wall)),
                          ms_per_trial_wall_spread=float(max(wall) - min(wall)), ms_per_trial_events=[r["ms_per_trial_events"] for r in rs],
                          it_per_s=[r["it_per_s"] for r in rs], accepted=[r["accepted"] for r in rs],
                          warmup_accepted=[r["warmup_accepted"] for r in rs], lr=rs[-1]["lr"])
        if len(runs) == 2:
            full = all(a == args.steps for k in runs for a in rec[k]["accepted"])
            rec["windows_all_accepted"] = full
            rec["multinomial_minus_logistic_ms_per_trial"] = (rec["multinomial"]["ms_per_trial_wall_median"]
                                                              - rec["logistic"]["ms_per_trial_wall_median"]) if full else None
            rec["multinomial_over_logistic"] = rec["multinomial"]["ms_per_trial_wall_median"] / rec["logistic"]["ms_per_trial_wall_median"]
            rec["summed_spread_ms"] = rec["multinomial"]["ms_per_trial_wall_spread"] + rec["logistic"]["ms_per_trial_wall_spread"]
        out["K"][str(K)] = rec
        print(f"K = {K} done at {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
