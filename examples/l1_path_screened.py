#!/usr/bin/env python3
"""A ten-point regularisation path of a sparse LASSO with gap-safe screening.

As examples/l1_path_sparse.py - one matrix in HBM, siblings (``with_lam``) warm-started along the path, every point stopped
on its duality gap - but each point is solved by ``zfista_amd.screening.solve_screened``: the gap evaluation also marks the
columns that are provably zero at the optimum, the matrix is restricted to the others on the device, and the solver runs on
that smaller problem.  The certificate of every point is the FULL problem's gap at the returned x.

    python examples/l1_path_screened.py [--m 20000 --n 50000 --density 0.001 --loss ls|logistic]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zfista_amd.path import l1_path  # noqa: E402
from zfista_amd.problems import SparseLeastSquaresL1, SparseLogisticL1  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--density", type=float, default=0.001)
    ap.add_argument("--loss", choices=("ls", "logistic"), default="ls")
    ap.add_argument("--points", type=int, default=10)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    A = sp.random(args.m, args.n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    x_true = np.zeros(args.n)
    x_true[rng.choice(args.n, 50, replace=False)] = rng.standard_normal(50)
    if args.loss == "logistic":
        b = np.sign(A @ x_true + 0.1 * rng.standard_normal(args.m))
        b[b == 0] = 1.0
        prob = SparseLogisticL1(A, b, 1.0)
    else:
        prob = SparseLeastSquaresL1(A, A @ x_true + 0.01 * rng.standard_normal(args.m), 1.0)
    lam_max = float(prob.lam_max())   # from here on up the solution is x = 0
    lams = lam_max * np.logspace(0, -2, args.points)
    gap_tol = 1e-6 * float(prob.with_lam(lams[-1]).duality_gap(np.zeros(args.n)).primal)
    t0 = time.time()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        path = l1_path(prob, lams, gap_tol=gap_tol, screen=True, lr=1.0, nesterov=True, tol=0.0, max_iter=5000)
    print(f"{args.m} x {args.n}, nnz {A.nnz}; lam_max {lam_max:.6g}; gap_tol {gap_tol:.3g}; {time.time() - t0:.2f} s")
    print(f"{'lam / lam_max':>14} {'nit':>6} {'checks':>6} {'gap':>12} {'F':>16} {'nonzeros':>9}  kept columns per round")
    for r in path:
        print(f"{r.lam / lam_max:14.5f} {r.nit:6d} {r.dual_gap_checks:6d} {r.dual_gap:12.4e} {float(r.fun):16.8e} "
              f"{np.count_nonzero(r.x):9d}  {[e['kept'] for e in r.screen]}")


if __name__ == "__main__":
    main()
