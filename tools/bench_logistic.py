#!/usr/bin/env python3
"""Rate of a device-resident L1 logistic-regression solve (LogisticL1 / SparseLogisticL1) beside its least-squares
sibling on the SAME matrix, one JSON line per process.

    python tools/bench_logistic.py --m 200000 --n 1000003 --per-col 8 --seed 7                  # SparseLogisticL1 | SparseLeastSquaresL1
    python tools/bench_logistic.py --m 8192 --n 32768 --density 0.01                           # the same, uniform density
    python tools/bench_logistic.py --m 16384 --n 65536 --backend dense --warmup 48             # LogisticL1 | LeastSquaresL1, A drawn in HBM
    python tools/bench_logistic.py --m 200000 --n 1000003 --per-col 8 --backend generic --steps 20   # SciPy closures, generic callback path
    python tools/bench_logistic.py ... --loss logistic --repeats 1                             # one class alone (a profiler run:
                                                                                               #  tools/trace_trials.py reads its trace)

The protocol is tools/bench_sparse.py's: the problem is seeded, built in this process and lives in HBM before anything is
timed; W untimed passes, a synchronise, K timed passes of NativeRun.advance, a synchronise; FISTA from lr = 1, one trial
per pass, so the W passes hold the backtracking.  --loss both (default) ALTERNATES the two classes `repeats` times in this
one process - ls, logistic, ls, logistic, ... - each run a fresh solver on the resident problem: the sibling's code is
the yardstick, and alternation keeps clocks and neighbours the same for both.  Labels are sign(A x_true + 0.1 noise),
lam a tenth of the smallest that gives x = 0 (for either loss), scale 1 (logistic) and 1/2 (least squares).

Reported per loss: ms per trial (wall) of every repeat with median and spread, accepted iterations per second, the
solver's own event time, the plan; the difference of the medians, only when every timed trial of both classes was accepted
(a rejected trial is followed by one without the A^T sweep: windows with rejections do not hold the same work - the dense
least-squares problem backtracks 22 times from lr = 1, so it is run with --warmup 48); and the ALGORITHMIC bytes of a logistic trial: the sibling's traffic model
(tools/bench_sparse.py) with the labels read twice - which it already counts as `b` in resid_y (32 m) and resid_x (16 m):
the loss kernels move the same bytes as the residual kernels they replace, and add ~150 fp64 instructions per row."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sparse import PEAK_BYTES_PER_S, algorithmic_bytes, lengths  # noqa: E402


def build_sparse(args):
    import scipy.sparse as sp

    rng = np.random.default_rng(args.seed)
    m, n = args.m, args.n
    if args.density is not None:
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
    b_ls = z + 0.01 * rng.standard_normal(m)
    labels = np.sign(z + 0.1 * rng.standard_normal(m))
    labels[labels == 0] = 1.0
    return A, b_ls, 0.1 * float(np.max(np.abs(A.T @ b_ls))), labels, 0.1 * float(np.max(np.abs(A.T @ (labels / 2))))


def build_dense(args):
    """A (m x n, N(0, 1)) drawn in HBM (8 GiB at 16384 x 65536: no host copy), the right-hand sides from it on the device."""
    import torch

    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    A = torch.randn(args.m, args.n, dtype=torch.float64, device="cuda", generator=gen)
    x_true = torch.zeros(args.n, dtype=torch.float64, device="cuda")
    k = min(200, args.n)
    x_true[torch.randperm(args.n, device="cuda", generator=gen)[:k]] = torch.randn(k, dtype=torch.float64, device="cuda", generator=gen)
    z = A @ x_true
    b_ls = z + 0.01 * torch.randn(args.m, dtype=torch.float64, device="cuda", generator=gen)
    labels = torch.sign(z + 0.1 * torch.randn(args.m, dtype=torch.float64, device="cuda", generator=gen))
    labels[labels == 0] = 1.0
    lam_ls = 0.1 * float(torch.max(torch.abs(A.T @ b_ls)))
    lam_lg = 0.1 * float(torch.max(torch.abs(A.T @ (labels / 2))))
    return A, b_ls, lam_ls, labels, lam_lg


def logistic_closures(A, b, lam):
    AT = A.T.tocsr()

    def terms(x):
        t = -b * (A @ x)
        return t, np.exp(-np.abs(t))

    def f(x):
        t, e = terms(x)
        return np.sum(np.maximum(t, 0.0) + np.log1p(e))

    def jac(x):
        t, e = terms(x)
        return AT @ (-b * (np.where(t >= 0, 1.0, e) / (1.0 + e)))

    return f, (lambda x: lam * np.linalg.norm(x, ord=1)), jac, (lambda w, x: np.sign(x) * np.maximum(np.abs(x) - lam * w, 0))


def timed_run(prob, n, warmup, steps, acceptance="reference"):
    import torch

    from zfista_amd.proximal_gradient import NativeRun

    opts = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=10 ** 9, max_iter_internal=100000, max_backtrack_iter=100,
                warm_start=False, decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False,
                deprecated=False, acceptance=acceptance)
    run = NativeRun(prob, np.zeros(n), opts, timing=True)
    plan = list(run.solver.ls_plan())
    warm = run.advance(warmup)
    run.solver.trial_kernel_ms()   # (resets the event window)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    rows = run.advance(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    ms, count = run.solver.trial_kernel_ms()
    run.solver.close()
    return dict(plan=plan, warmup_accepted=len(warm), accepted=len(rows), seconds=dt, it_per_s=len(rows) / dt,
                ms_per_trial_wall=1e3 * dt / steps, ms_per_trial_events=ms, timed_launches=int(count),
                lr=float(rows[-1][2]) if len(rows) else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--backend", choices=("sparse", "dense", "generic"), default="sparse")
    ap.add_argument("--loss", choices=("both", "logistic", "ls"), default="both")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--label", default="")
    ap.add_argument("--acceptance", choices=("reference", "remainder"), default="reference",
                    help="acceptance test of the LEAST-SQUARES sibling (the logistic classes have the reference's only; DESIGN 4.4)")
    args = ap.parse_args()

    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.problems import LeastSquaresL1, LogisticL1, SparseLeastSquaresL1, SparseLogisticL1

    t0 = time.time()
    A, b_ls, lam_ls, labels, lam_lg = build_dense(args) if args.backend == "dense" else build_sparse(args)
    m, n = int(A.shape[0]), int(A.shape[1])
    out = dict(tool="bench_logistic", label=args.label, backend=args.backend, loss=args.loss, ls_acceptance=args.acceptance, m=m, n=n, seed=args.seed,
               warmup=args.warmup, steps=args.steps, repeats=args.repeats, build_s=round(time.time() - t0, 2))
    if args.backend != "dense":
        out.update(nnz=int(A.nnz), row_len_A=lengths(A.indptr), row_len_At=lengths(A.T.tocsr().indptr))
    print(f"built {m} x {n} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    if args.backend == "generic":
        # what a user with +-1 labels gets without the native classes: NumPy / SciPy closures, a host round trip each
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t1 = time.time()
            res = minimize_proximal_gradient(*logistic_closures(A, labels, lam_lg), np.zeros(n), lr=1, tol=0.0, nesterov=True,
                                             max_iter=args.steps)
            dt = time.time() - t1
        out.update(iterations=int(res.nit), seconds=dt, it_per_s=res.nit / dt)
        print(json.dumps(out))
        return
    sparse = args.backend == "sparse"
    probs = {}
    if args.loss in ("both", "ls"):
        probs["ls"] = SparseLeastSquaresL1(A, b_ls, lam_ls) if sparse else LeastSquaresL1(A, b_ls, lam_ls)
    if args.loss in ("both", "logistic"):
        probs["logistic"] = SparseLogisticL1(A, labels, lam_lg) if sparse else LogisticL1(A, labels, lam_lg)
    runs = {k: [] for k in probs}
    for _ in range(args.repeats):
        for k, prob in probs.items():   # alternated: ls, logistic, ls, logistic, ...
            runs[k].append(timed_run(prob, n, args.warmup, args.steps, args.acceptance if k == "ls" else "reference"))
    for k, rs in runs.items():
        wall = [r["ms_per_trial_wall"] for r in rs]
        out[k] = dict(plan=rs[0]["plan"], ms_per_trial_wall=wall, ms_per_trial_wall_median=float(np.median(wall)),
                      ms_per_trial_wall_spread=float(max(wall) - min(wall)), ms_per_trial_events=[r["ms_per_trial_events"] for r in rs],
                      it_per_s=[r["it_per_s"] for r in rs], accepted=[r["accepted"] for r in rs],
                      warmup_accepted=[r["warmup_accepted"] for r in rs], lr=rs[-1]["lr"])
    if len(runs) == 2:
        # the two windows hold the same work only when every timed trial of both was accepted: the trial after a rejected
        # one skips the A^T sweep.  Otherwise no difference is reported (raise --warmup until the line search has settled).
        full = all(a == args.steps for k in runs for a in out[k]["accepted"])
        out["windows_all_accepted"] = full
        out["logistic_minus_ls_ms_per_trial"] = (out["logistic"]["ms_per_trial_wall_median"] - out["ls"]["ms_per_trial_wall_median"]
                                                 if full else None)
    if sparse:
        nbytes = algorithmic_bytes(m, n, int(A.nnz))
        out["algorithmic_bytes_per_trial"] = nbytes
        if "logistic" in out:
            out["logistic_fraction_of_8TBps"] = nbytes / (1e-3 * out["logistic"]["ms_per_trial_wall_median"]) / PEAK_BYTES_PER_S
    else:
        out["dense_bytes_per_sweep"] = 8 * m * n
    print(json.dumps(out))


if __name__ == "__main__":
    main()
