#!/usr/bin/env python3
"""Choosing the l1 weight by K-fold cross-validation on ONE device-resident matrix.

``l1_path`` gives a path; ``l1_cv`` picks a point on it.  A fold is the same matrix with 0 / 1 row weights
(``problem.with_sample_weight``): the K training problems, the K held-out scores and the final fit all share one upload of A -
only m-vectors of weights go to HBM.  The same weights serve class imbalance, replicated observations and rows to be ignored;
here a tenth of the rows is given weight 0 up front (say, rows known to be corrupt) and the folds respect that.

    python examples/l1_cv.py [--m 20000 --n 2000 --density 0.01 --points 8 --folds 5 --loss ls|logistic]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zfista_amd.path import l1_cv  # noqa: E402
from zfista_amd.problems import SparseLeastSquaresL1, SparseLogisticL1  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--loss", choices=("ls", "logistic"), default="ls")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    A = sp.random(args.m, args.n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    x_true = np.zeros(args.n)
    support = rng.choice(args.n, 20, replace=False)
    x_true[support] = rng.standard_normal(20)
    z = A @ x_true
    w = np.ones(args.m)
    w[rng.choice(args.m, args.m // 10, replace=False)] = 0.0   # rows to be ignored: not there, for training and for scoring
    if args.loss == "logistic":
        b = np.where(z + 0.1 * rng.standard_normal(args.m) >= 0, 1.0, -1.0)
        prob = SparseLogisticL1(A, b, 1.0).with_sample_weight(w)
    else:
        b = z + 0.05 * rng.standard_normal(args.m)
        b[w == 0] += 10.0   # (what the ignored rows hold does not matter)
        prob = SparseLeastSquaresL1(A, b, 1.0, sample_weight=w)
    lam_max = float(prob.lam_max())
    lams = lam_max * np.logspace(-0.05, -2.5, args.points)
    gap_tol = 1e-5 * float(prob.with_lam(lams[-1]).duality_gap(np.zeros(args.n)).primal)
    print(f"{args.m} x {args.n}, nnz {A.nnz}; {int((w == 0).sum())} rows of weight 0; lam_max {lam_max:.6g}, gap_tol {gap_tol:.3g}")
    t0 = time.time()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cv = l1_cv(prob, lams, folds=args.folds, seed=0, gap_tol=gap_tol, lr=1.0, nesterov=True, tol=0.0, max_iter=5000)
    print(f"{args.folds} folds x {args.points} points and the fit on all rows: {time.time() - t0:.2f} s on one upload of A\n")
    print(f"{'lam / lam_max':>14} {'held-out loss':>14} {'+- se':>10} {'nonzeros':>9} {'of the true support':>19}")
    for l, r in enumerate(cv.path):
        nz = np.flatnonzero(r.x)
        mark = " <- best" if l == cv.best else (" <- 1 se" if cv.lams[l] == cv.lam_1se else "")
        print(f"{cv.lams[l] / lam_max:14.5f} {cv.mean[l]:14.6g} {cv.se[l]:10.3g} {nz.size:9d} {int(np.isin(nz, support).sum()):19d}{mark}")
    print(f"\nlam_best = {cv.lam_best:.6g}, lam_1se = {cv.lam_1se:.6g}")


if __name__ == "__main__":
    main()
