#!/usr/bin/env python3
"""Rate of a device-resident Poisson solve (PoissonL1 / SparsePoissonL1) beside its least-squares sibling on the SAME matrix, one
JSON line per process.

    python tools/bench_poisson.py --m 200000 --n 1000003 --per-col 8 --seed 7           # SparsePoissonL1 | SparseLeastSquaresL1
    python tools/bench_poisson.py --m 8192 --n 32768 --density 0.01                     # the same, uniform density
    python tools/bench_poisson.py --m 16384 --n 65536 --backend dense --repeats 5       # PoissonL1 | LeastSquaresL1, A drawn in HBM
    python tools/bench_poisson.py ... --loss poisson --repeats 1                        # one class alone (a profiler run:
                                                                                        #  tools/trace_trials.py reads its trace)
    python tools/bench_poisson.py ... --loss logistic --repeats 1                       # the logistic class on the same matrix: its row
                                                                                        #  kernels are the second yardstick

The protocol is tools/bench_huber.py's (the builders and the timed window of tools/bench_logistic.py are imported): the problem is
seeded, built in this process and lives in HBM before anything is timed; W untimed passes, a synchronise, K timed passes of
NativeRun.advance, a synchronise; FISTA from lr = 1, one trial per pass.  --loss both (default) ALTERNATES the two classes
`repeats` times in this one process - ls, poisson, ls, poisson, ... - each run a fresh solver on the resident problem.

So that the line search has settled before the timed window at W = 16, both losses are means over the rows: scale = 1 / m for
the Poisson class and 1 / (2 m) for the least-squares sibling (from lr = 1 a dense 16384 x 65536 N(0, 1) matrix needs 4
halvings then instead of 18).  The counts are b ~ Poisson(exp(clip((A x_true) / 4, -30, 2))), drawn once from the seed; lam is
a tenth of the smallest that gives x = 0 for the class.

Reported per loss: ms per trial (wall) of every repeat with median and spread, accepted iterations per second, the solver's own
event time, the plan; the difference of the medians, only when every timed trial of both classes was accepted (a rejected trial
is followed by one without the A^T sweep: windows with rejections do not hold the same work).  The rule of DESIGN 4.5c: a Poisson
trial may exceed a sibling trial by at most (Poisson row kernels - residual kernels, from one kernel trace per class) + the
summed spread of the two sets of repeats.  The loss kernels move the bytes of the residual kernels they replace (32 m at y,
16 m at x+)."""
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


def draw_counts(b_ls, seed):
    """Counts ~ Poisson(exp(clip(z / 4, -30, 2))) with z the least-squares right-hand side (A x_true + noise); a host array or a
    CUDA tensor, as b_ls is."""
    if isinstance(b_ls, np.ndarray):
        rng = np.random.default_rng(seed + 2000)
        return rng.poisson(np.exp(np.clip(b_ls / 4.0, -30.0, 2.0))).astype(np.float64)
    import torch

    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed + 2000)
    return torch.poisson(torch.exp(torch.clamp(b_ls / 4.0, -30.0, 2.0)), generator=gen)


def lam_tenth(A, cand, scale):
    """0.1 scale |A^T cand|_inf: a tenth of the smallest lam that gives x = 0 (grad f(0) = scale A^T cand up to its sign)."""
    if isinstance(cand, np.ndarray):
        return 0.1 * scale * float(np.max(np.abs(A.T @ cand)))
    return 0.1 * scale * float((A.T @ cand).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--backend", choices=("sparse", "dense"), default="sparse")
    ap.add_argument("--loss", choices=("both", "poisson", "ls", "logistic"), default="both")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    from zfista_amd.problems import LeastSquaresL1, LogisticL1, PoissonL1, SparseLeastSquaresL1, SparseLogisticL1, SparsePoissonL1

    t0 = time.time()
    A, b_ls, _, labels, _ = build_dense(args) if args.backend == "dense" else build_sparse(args)
    counts = draw_counts(b_ls, args.seed)
    m, n = int(A.shape[0]), int(A.shape[1])
    scale_p, scale_ls = 1.0 / m, 0.5 / m
    lam_p, lam_ls, lam_lg = lam_tenth(A, 1.0 - counts, scale_p), lam_tenth(A, b_ls, 2 * scale_ls), lam_tenth(A, labels / 2, scale_p)
    out = dict(tool="bench_poisson", label=args.label, backend=args.backend, loss=args.loss, m=m, n=n, seed=args.seed, warmup=args.warmup,
               steps=args.steps, repeats=args.repeats, scale_poisson=scale_p, scale_ls=scale_ls, lam_ls=lam_ls, lam_poisson=lam_p,
               max_count=float(counts.max()), zero_share=float((counts == 0).sum()) / m, build_s=round(time.time() - t0, 2))
    sparse = args.backend == "sparse"
    if sparse:
        out.update(nnz=int(A.nnz), row_len_A=lengths(A.indptr), row_len_At=lengths(A.T.tocsr().indptr))
    print(f"built {m} x {n} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    probs = {}
    if args.loss in ("both", "ls"):
        probs["ls"] = SparseLeastSquaresL1(A, b_ls, lam_ls, scale=scale_ls) if sparse else LeastSquaresL1(A, b_ls, lam_ls, scale=scale_ls)
    if args.loss in ("both", "poisson"):
        probs["poisson"] = SparsePoissonL1(A, counts, lam_p, scale=scale_p) if sparse else PoissonL1(A, counts, lam_p, scale=scale_p)
    if args.loss == "logistic":
        probs["logistic"] = SparseLogisticL1(A, labels, lam_lg, scale=scale_p) if sparse else LogisticL1(A, labels, lam_lg, scale=scale_p)
    runs = {k: [] for k in probs}
    for _ in range(args.repeats):
        for k, prob in probs.items():   # alternated: ls, poisson, ls, poisson, ...
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
        out["poisson_minus_ls_ms_per_trial"] = (out["poisson"]["ms_per_trial_wall_median"] - out["ls"]["ms_per_trial_wall_median"]) if full else None
        out["summed_spread_ms"] = out["poisson"]["ms_per_trial_wall_spread"] + out["ls"]["ms_per_trial_wall_spread"]
    if sparse:
        nbytes = algorithmic_bytes(m, n, int(A.nnz))
        out["algorithmic_bytes_per_trial"] = nbytes
        if "poisson" in out:
            out["poisson_fraction_of_8TBps"] = nbytes / (1e-3 * out["poisson"]["ms_per_trial_wall_median"]) / PEAK_BYTES_PER_S
    else:
        out["dense_bytes_per_sweep"] = 8 * m * n
    print(json.dumps(out))


if __name__ == "__main__":
    main()
