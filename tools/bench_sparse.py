#!/usr/bin/env python3
"""Rate of a device-resident sparse LASSO solve (SparseLeastSquaresL1), one JSON line per process.

    python tools/bench_sparse.py --m 200000 --n 1000003 --per-col 8 --seed 7 --warmup 16 --steps 64
    python tools/bench_sparse.py ... --skew                 # + one dense row and one dense column
    python tools/bench_sparse.py --m 8192 --n 32768 --density 0.01 --backend dense     # LeastSquaresL1 on A.toarray()
    python tools/bench_sparse.py ... --backend generic --steps 20    # SciPy closures through the generic callback path

The problem is seeded (the recipe of the tests' large case: `per_col` draws per column, duplicates summed; or a uniform
`density`), built in this process, and lives in HBM before anything is timed.  W untimed passes, a synchronise, K timed
passes of NativeRun.advance, a synchronise: FISTA from lr = 1, one trial per pass, so the W passes hold the
backtracking.  Reported: shape, nnz, row-length min / median / max of A and A^T, the plan (zf_solver_ls_plan), accepted
iterations per second, ms per trial from the solver's own events (the sparse kind brackets the whole trial), and the
ALGORITHMIC bytes of an accepted iteration with their fraction of 8 TB/s:

    sweeps   (12 nnz + 8 m + 8) + (12 nnz + 8 n + 8)   values + indices once and a row pointer per row, for A and for A^T
             + 8 m + 8 n                               their outputs s+ and grad
    shared   resid_y 32 m (s_k, s_{k-1}, b in, r out), prox step 32 n (x_k, x_{k-1}, grad in, x+ out; 24 n without
             momentum), resid_x 16 m (s+, b)

The gathered vectors (x+ for A, r for A^T) are served by the caches and are not counted."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8e12


def build(args):
    import scipy.sparse as sp

    rng = np.random.default_rng(args.seed)
    m, n = args.m, args.n
    if args.density is not None:
        A = sp.random(m, n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    else:
        rows = rng.integers(0, m, n * args.per_col)
        cols = np.repeat(np.arange(n), args.per_col)
        A = sp.csr_matrix((rng.standard_normal(n * args.per_col), (rows, cols)), shape=(m, n))
    if args.skew:   # an intercept-like dense column and one dense row, on top of the same matrix
        extra = sp.coo_matrix((rng.standard_normal(n), (np.full(n, m // 3), np.arange(n))), shape=(m, n)) + \
                sp.coo_matrix((rng.standard_normal(m), (np.arange(m), np.full(m, n // 5))), shape=(m, n))
        A = (A + extra.tocsr()).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    x_true = np.zeros(n)
    k = min(200, n)
    x_true[rng.choice(n, k, replace=False)] = rng.standard_normal(k)
    b = A @ x_true + 0.01 * rng.standard_normal(m)
    return A, b, 0.1 * float(np.max(np.abs(A.T @ b)))


def lengths(indptr):
    d = np.diff(indptr)
    return [int(d.min()), float(np.median(d)), int(d.max())]


def algorithmic_bytes(m, n, nnz, nesterov=True):
    sweeps = 2 * (12 * nnz + 8) + 8 * (m + n) + 8 * m + 8 * n
    shared = 32 * m + (32 if nesterov else 24) * n + 16 * m
    return sweeps + shared


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--skew", action="store_true")
    ap.add_argument("--backend", choices=("sparse", "dense", "generic"), default="sparse")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--label", default="")
    ap.add_argument("--acceptance", choices=("reference", "remainder"), default="reference",
                    help="how the sufficient-decrease test is evaluated (native backends; DESIGN 4.4)")
    ap.add_argument("--repeats", type=int, default=1, help="timed solves of the same problem (native backends)")
    args = ap.parse_args()

    import torch

    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.problems import LeastSquaresL1, SparseLeastSquaresL1
    from zfista_amd.proximal_gradient import NativeRun

    t0 = time.time()
    A, b, lam = build(args)
    m, n = A.shape
    print(f"built {m} x {n}, nnz {A.nnz} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    out = dict(tool="bench_sparse", label=args.label, backend=args.backend, acceptance=args.acceptance, m=m, n=n, nnz=int(A.nnz), skew=bool(args.skew),
               seed=args.seed, row_len_A=lengths(A.indptr), row_len_At=lengths(A.T.tocsr().indptr),
               warmup=args.warmup, steps=args.steps, build_s=round(time.time() - t0, 2))
    if args.backend == "generic":
        # what a user with a sparse matrix gets without the native class: NumPy / SciPy closures, a host round trip each
        AT = A.T.tocsr()
        cb = (lambda x: 0.5 * np.linalg.norm(A @ x - b) ** 2, lambda x: lam * np.linalg.norm(x, ord=1),
              lambda x: AT @ (A @ x - b), lambda w, x: np.sign(x) * np.maximum(np.abs(x) - lam * w, 0))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t1 = time.time()
            res = minimize_proximal_gradient(*cb, np.zeros(n), lr=1, tol=0.0, nesterov=True, max_iter=args.steps)
            dt = time.time() - t1
        out.update(iterations=int(res.nit), seconds=dt, it_per_s=res.nit / dt)
        print(json.dumps(out))
        return
    prob = SparseLeastSquaresL1(A, b, lam) if args.backend == "sparse" else LeastSquaresL1(A.toarray(), b, lam)
    opts = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=10 ** 9, max_iter_internal=100000, max_backtrack_iter=100,
                warm_start=False, decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False,
                deprecated=False, acceptance=args.acceptance)
    walls = []
    for rep_no in range(max(1, args.repeats)):   # (the figures reported below are the last repeat's; every repeat's wall time is kept)
        if rep_no:
            run.solver.close()
        run = NativeRun(prob, np.zeros(n), opts, timing=True)
        out["plan"] = list(run.solver.ls_plan())
        warm = run.advance(args.warmup)
        run.solver.trial_kernel_ms()   # (resets the event window)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rows = run.advance(args.steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        ms, count = run.solver.trial_kernel_ms()
        accepted = len(rows)
        walls.append(dict(ms_per_trial_wall=1e3 * dt / args.steps, accepted=accepted))
    if args.repeats > 1:
        out["repeats"] = walls
    out.update(warmup_accepted=len(warm), accepted=accepted, trials=args.steps, seconds=dt, it_per_s=accepted / dt,
               ms_per_trial_wall=1e3 * dt / args.steps, ms_per_trial_events=ms, timed_launches=int(count),
               lr=float(rows[-1][2]) if accepted else None)
    if args.backend == "sparse":
        nbytes = algorithmic_bytes(m, n, int(A.nnz))
        out.update(algorithmic_bytes_per_iteration=nbytes,
                   fraction_of_8TBps=nbytes * accepted / dt / PEAK_BYTES_PER_S)
    else:
        out.update(dense_bytes_per_sweep=8 * m * n)
    run.solver.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
