#!/usr/bin/env python3
"""Screened against unscreened regularisation paths on one device-resident matrix, one JSON line per process.

    python tools/bench_screen.py --m 200000 --n 1000003 --per-col 8 --seed 7                    # sparse least squares
    python tools/bench_screen.py --m 200000 --n 1000003 --per-col 8 --seed 7 --loss logistic
    python tools/bench_screen.py --m 8192 --n 32768 --density 0.01 --screen-ratio 0.3

The seeded problem (tools/bench_gap.py's) lives in HBM before anything is timed.  The path is lam_max * logspace(0, -2, points),
every point solved to gap_tol = `--gap-rel` times P(0) of the last point, warm-started.  `--repeats` alternated pairs of
l1_path(screen=True) and l1_path(screen=False) after one untimed pair: wall time per path, nit and kept columns per lam.
Beside them, the cost of the pieces with the trial of the same matrix as the yardstick (NativeRun.advance after its warm-up,
as tools/bench_gap.py): ms per trial, per problem.screen(x), per problem.duality_gap(x) and per problem.restrict(keep) at the
kept set of the middle point of the path."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_gap import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--backend", choices=("sparse", "dense"), default="sparse")
    ap.add_argument("--loss", choices=("ls", "logistic"), default="ls")
    ap.add_argument("--points", type=int, default=10)
    ap.add_argument("--gap-rel", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--screen-ratio", type=float, default=0.1)
    ap.add_argument("--screen-shrink", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pieces", type=int, default=8, help="timed calls of each piece")
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch

    from zfista_amd import problems as Z
    from zfista_amd.path import l1_path
    from zfista_amd.proximal_gradient import NativeRun

    t0 = time.time()
    A, b, lam0 = build(args)
    m, n = A.shape
    cls = {("sparse", "ls"): Z.SparseLeastSquaresL1, ("sparse", "logistic"): Z.SparseLogisticL1,
           ("dense", "ls"): Z.LeastSquaresL1, ("dense", "logistic"): Z.LogisticL1}[(args.backend, args.loss)]
    prob = cls(A, b, lam0)
    lam_max = float(prob.lam_max())
    lams = lam_max * np.logspace(0, -2, args.points)
    gap_tol = args.gap_rel * float(prob.with_lam(lams[-1]).duality_gap(np.zeros(n)).primal)
    out = dict(tool="bench_screen", label=args.label, backend=args.backend, loss=args.loss, m=m, n=n,
               nnz=int(A.nnz) if args.backend == "sparse" else m * n, seed=args.seed, points=args.points, gap_tol=gap_tol,
               lam_max=lam_max, screen_ratio=args.screen_ratio, screen_shrink=args.screen_shrink, max_iter=args.max_iter,
               build_s=round(time.time() - t0, 2))
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=args.max_iter)
    skw = dict(kw, screen_ratio=args.screen_ratio, screen_shrink=args.screen_shrink)

    def one(screen):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            path = l1_path(prob, lams, gap_tol=gap_tol, screen=screen, **(skw if screen else kw))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t1), path

    one(True), one(False)   # (first touch: module load, allocator, the norms)
    pairs = []
    for _ in range(args.repeats):
        ms_s, ps = one(True)
        ms_p, pp = one(False)
        pairs.append(dict(screened_ms=ms_s, plain_ms=ms_p))
    out.update(pairs=pairs, screened_ms_median=float(np.median([p["screened_ms"] for p in pairs])),
               plain_ms_median=float(np.median([p["plain_ms"] for p in pairs])))
    out["speedup"] = out["plain_ms_median"] / out["screened_ms_median"]
    out["per_lam"] = [dict(lam_over_lam_max=float(r.lam / lam_max), nit_screened=int(r.nit), nit_plain=int(q.nit),
                           gap_screened=float(r.dual_gap), gap_plain=float(q.dual_gap), success=bool(r.success and q.success),
                           nonzeros=int(np.count_nonzero(r.x)), rounds=len(r.screen),
                           kept=[int(e["kept"]) for e in r.screen], restricted=[bool(e["restricted"]) for e in r.screen],
                           fun_diff=float(abs(r.fun - q.fun)))
                      for r, q in zip(ps, pp)]
    # the pieces beside a trial of the same matrix
    mid = ps[len(ps) // 2]
    sib = prob.with_lam(mid.lam)
    opts = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=10 ** 9, max_iter_internal=100000, max_backtrack_iter=100,
                warm_start=False, decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False,
                deprecated=False)
    run = NativeRun(sib, np.zeros(n), opts, timing=True)
    run.advance(16)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    run.advance(64)
    torch.cuda.synchronize()
    trial_ms = 1e3 * (time.perf_counter() - t1) / 64
    run.solver.close()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.pieces):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t1) / args.pieces

    sc = sib.screen(mid.x)
    out.update(ms_per_trial=trial_ms, ms_per_screen=timed(lambda: sib.screen(mid.x)), ms_per_gap=timed(lambda: sib.duality_gap(mid.x)),
               ms_per_restrict=timed(lambda: sib.restrict(sc)) if sc.count else None, restrict_kept=int(sc.count),
               restrict_nnz=int(sib.restrict(sc).nnz) if sc.count and args.backend == "sparse" else None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
