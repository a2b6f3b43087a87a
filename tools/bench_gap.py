#!/usr/bin/env python3
"""Cost of a duality-gap check beside a trial of the same device-resident solve, one JSON line per process.

    python tools/bench_gap.py --m 200000 --n 1000003 --per-col 8 --seed 7                    # sparse least squares
    python tools/bench_gap.py --m 200000 --n 1000003 --per-col 8 --seed 7 --loss logistic
    python tools/bench_gap.py --m 8192 --n 32768 --density 0.01
    python tools/bench_gap.py --m 16384 --n 65536 --backend dense                            # a dense normal matrix

The protocol of tools/bench_sparse.py: the seeded problem lives in HBM before anything is timed; W = 16 untimed passes (they
hold the backtracking of the lr = 1 start), a synchronise, K = 64 timed passes of NativeRun.advance, a synchronise; then 64
timed NativeRun.duality_gap() calls (each synchronises: a check as a solve with gap_tol pays it).  Reported: ms per trial,
ms per gap check, their ratio, the gap.  A check is the A^T sweep and the residual / loss kernel of a trial plus the new
kernels of csrc/zf_kernels_gap.h, whose bytes are 8 n (|g|_inf) + 16 n (columns) + 16 m (logistic rows) (+ 24 m: r, least squares).

--stopping: the overhead of gap_tol itself - `--repeats` alternated pairs of the same solve of W + K passes without the keyword
and with gap_tol = 0, gap_every = 16 (one check per 16 trials, never stopping), median ms per trial of each.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_gap.py ...` for the per-kernel durations."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(args):
    import scipy.sparse as sp

    rng = np.random.default_rng(args.seed)
    m, n = args.m, args.n
    if args.backend == "dense":
        A = rng.standard_normal((m, n))
    elif args.density is not None:
        A = sp.random(m, n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    else:
        rows = rng.integers(0, m, n * args.per_col)
        cols = np.repeat(np.arange(n), args.per_col)
        A = sp.csr_matrix((rng.standard_normal(n * args.per_col), (rows, cols)), shape=(m, n))
        A.sum_duplicates()
        A.sort_indices()
    x_true = np.zeros(n)
    k = min(200, n)
    x_true[rng.choice(n, k, replace=False)] = rng.standard_normal(k)
    z = A @ x_true
    if args.loss == "logistic":
        b = np.sign(z + 0.1 * rng.standard_normal(m))
        b[b == 0] = 1.0
        return A, b, 0.1 * float(np.max(np.abs(A.T @ (b / 2))))
    b = z + 0.01 * rng.standard_normal(m)
    return A, b, 0.1 * float(np.max(np.abs(A.T @ b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--backend", choices=("sparse", "dense"), default="sparse")
    ap.add_argument("--loss", choices=("ls", "logistic"), default="ls")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--checks", type=int, default=64)
    ap.add_argument("--stopping", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch

    from zfista_amd import minimize_proximal_gradient, problems as Z
    from zfista_amd.proximal_gradient import NativeRun

    t0 = time.time()
    A, b, lam = build(args)
    m, n = A.shape
    cls = {("sparse", "ls"): Z.SparseLeastSquaresL1, ("sparse", "logistic"): Z.SparseLogisticL1,
           ("dense", "ls"): Z.LeastSquaresL1, ("dense", "logistic"): Z.LogisticL1}[(args.backend, args.loss)]
    prob = cls(A, b, lam)
    out = dict(tool="bench_gap", label=args.label, backend=args.backend, loss=args.loss, m=m, n=n,
               nnz=int(A.nnz) if args.backend == "sparse" else m * n, seed=args.seed, warmup=args.warmup, steps=args.steps,
               build_s=round(time.time() - t0, 2))
    new_bytes = 24 * n + (16 * m if args.loss == "logistic" else 24 * m)
    out["new_kernel_bytes"] = new_bytes
    if args.stopping:
        kw = dict(lr=1, tol=0.0, nesterov=True, max_iter=args.warmup + args.steps)
        pairs = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            minimize_proximal_gradient(*prob.callbacks(), np.zeros(n), **kw)   # (first touch: module load, allocator)
            for _ in range(args.repeats):
                pair = {}
                for name, extra in (("plain", {}), ("gap_tol", dict(gap_tol=0.0, gap_every=16))):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    res = minimize_proximal_gradient(*prob.callbacks(), np.zeros(n), **kw, **extra)
                    torch.cuda.synchronize()
                    pair[name] = 1e3 * (time.perf_counter() - t1)
                    pair[name + "_nit"] = int(res.nit)
                    if extra:
                        pair["checks"] = int(res.dual_gap_checks)
                pairs.append(pair)
        plain = float(np.median([p["plain"] for p in pairs]))
        gapped = float(np.median([p["gap_tol"] for p in pairs]))
        out.update(mode="stopping", pairs=pairs, solve_ms_plain_median=plain, solve_ms_gap_tol_median=gapped,
                   overhead=gapped / plain - 1.0)
        print(json.dumps(out))
        return
    opts = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=10 ** 9, max_iter_internal=100000, max_backtrack_iter=100,
                warm_start=False, decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False,
                deprecated=False)
    run = NativeRun(prob, np.zeros(n), opts, timing=True)
    out["plan"] = list(run.solver.ls_plan())
    run.advance(args.warmup)
    run.duality_gap()   # (the workspace is allocated by the first call)
    trial_ms = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rows = run.advance(args.steps)
        torch.cuda.synchronize()
        trial_ms.append(1e3 * (time.perf_counter() - t1) / args.steps)
    check_ms = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.checks):
            gp = run.duality_gap()
        torch.cuda.synchronize()
        check_ms.append(1e3 * (time.perf_counter() - t1) / args.checks)
    out.update(mode="check", accepted_last=len(rows), ms_per_trial=trial_ms, ms_per_gap_check=check_ms,
               ms_per_trial_median=float(np.median(trial_ms)), ms_per_gap_check_median=float(np.median(check_ms)),
               check_over_trial=float(np.median(check_ms) / np.median(trial_ms)), gap=float(gp.gap), primal=float(gp.primal),
               alpha=float(gp.alpha), stopping_model_overhead=float(np.median(check_ms) / np.median(trial_ms)) / 16)
    run.solver.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
