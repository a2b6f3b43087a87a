#!/usr/bin/env python3
"""An elastic-net regularisation path on one device-resident matrix with groups of correlated columns.

With correlated columns the plain LASSO keeps one column of a group, and which one changes along the path; the ridge term
(l2 / 2) |x|^2 spreads the weight over the group.  The matrix goes to HBM once; every point is a sibling problem
(``with_penalty``) that shares it, warm-started from the point before and stopped on the elastic-net duality gap.

    python examples/enet_path.py [--m 20000 --n 50000 --density 0.001 --loss ls|logistic --ratio 0.5]
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
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--ratio", type=float, default=0.5, help="l2 = ratio * lam at every point of the path")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    A = sp.random(args.m, args.n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    group = np.arange(0, 40, 2)   # columns 2k + 1 are noisy copies of columns 2k: twenty correlated pairs
    for j in group:
        A[:, j + 1] = A[:, j] + 0.05 * sp.random(args.m, 1, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    A = A.tocsr()
    x_true = np.zeros(args.n)
    x_true[group] = x_true[group + 1] = rng.standard_normal(group.size)
    if args.loss == "logistic":
        b = np.sign(A @ x_true + 0.1 * rng.standard_normal(args.m))
        b[b == 0] = 1.0
        prob = SparseLogisticL1(A, b, 1.0)
    else:
        prob = SparseLeastSquaresL1(A, A @ x_true + 0.01 * rng.standard_normal(args.m), 1.0)
    lam_max = float(prob.lam_max())   # unchanged by the ridge term, which vanishes at x = 0
    lams = lam_max * np.logspace(0, -1.5, args.points)
    gap_tol = 1e-6 * float(prob.with_lam(lams[-1]).duality_gap(np.zeros(args.n)).primal)
    kw = dict(gap_tol=gap_tol, lr=1.0, nesterov=True, tol=0.0, max_iter=5000)
    print(f"{args.m} x {args.n}, nnz {A.nnz}; lam_max {lam_max:.6g}; gap_tol {gap_tol:.3g}")
    for name, l2 in (("lasso", None), (f"elastic net, l2 = {args.ratio} lam", args.ratio * lams)):
        t0 = time.time()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            path = l1_path(prob, lams, l2=l2, **kw)
        print(f"\n{name}: {time.time() - t0:.2f} s")
        print(f"{'lam / lam_max':>14} {'nit':>6} {'gap':>12} {'F':>16} {'nonzeros':>9} {'pairs with both columns':>24}")
        for r in path:
            both = int(np.count_nonzero((r.x[group] != 0) & (r.x[group + 1] != 0)))
            print(f"{r.lam / lam_max:14.5f} {r.nit:6d} {r.dual_gap:12.4e} {float(r.fun):16.8e} {np.count_nonzero(r.x):9d} {both:24d}")


if __name__ == "__main__":
    main()
