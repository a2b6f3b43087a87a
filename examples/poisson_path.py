#!/usr/bin/env python3
"""An L1 path and a K-fold cross-validation of Poisson regression with an exposure vector.

Row i was observed for a time t_i and counted c_i ~ Poisson(t_i exp((A x)_i)) events.  Its negative log-likelihood is
t_i exp(z_i) - c_i z_i up to a constant = t_i (exp(z_i) - (c_i / t_i) z_i): the Poisson loss of the RATE c_i / t_i with the
sample weight t_i.  So the exposure needs no offset column and no extra machinery: ``SparsePoissonL1(A, c / t, lam,
sample_weight=t)``.  The matrix goes to HBM once; every point of the path is a sibling problem (``with_lam``) that shares it,
warm-started from the point before and stopped on its duality gap; every fold of ``l1_cv`` is a 0 / 1-weighted sibling.

    python examples/poisson_path.py [--m 20000 --n 2000 --density 0.01 --points 8 --folds 5]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zfista_amd.path import l1_cv, l1_path  # noqa: E402
from zfista_amd.problems import SparsePoissonL1  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--folds", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    A = sp.random(args.m, args.n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    x_true = np.zeros(args.n)
    support = rng.choice(args.n, 20, replace=False)
    x_true[support] = 0.5 * rng.standard_normal(20)
    exposure = rng.uniform(0.25, 4.0, args.m)
    counts = rng.poisson(exposure * np.exp(np.clip(A @ x_true, -30.0, 6.0))).astype(np.float64)
    prob = SparsePoissonL1(A, counts / exposure, 1.0, scale=1.0 / exposure.sum(), sample_weight=exposure)
    lam_max = float(prob.lam_max())
    lams = lam_max * np.logspace(0, -1.5, args.points)
    gap_tol = 1e-6 * float(prob.with_lam(lams[-1]).duality_gap(np.zeros(args.n)).primal)
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=5000)
    print(f"{args.m} x {args.n}, nnz {A.nnz}; counts up to {int(counts.max())}, {np.mean(counts == 0):.0%} zeros; exposure 0.25 .. 4")
    t0 = time.time()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        path = l1_path(prob, lams, gap_tol=gap_tol, **kw)
    print(f"\npath: lam_max {lam_max:.6g}, gap_tol {gap_tol:.3g}, {time.time() - t0:.2f} s")
    print(f"{'lam / lam_max':>14} {'nit':>6} {'gap':>12} {'nonzeros':>9} {'of the true support':>19} {'|x - x_true|_2':>15}")
    for r in path:
        nz = np.flatnonzero(r.x)
        hit = int(np.isin(nz, support).sum())
        print(f"{r.lam / lam_max:14.5f} {r.nit:6d} {r.dual_gap:12.4e} {nz.size:9d} {hit:19d} {np.linalg.norm(r.x - x_true):15.6f}")
    t0 = time.time()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cv = l1_cv(prob, lams, folds=args.folds, seed=0, gap_tol=gap_tol, refit=False, **kw)
    print(f"\nl1_cv, {args.folds} folds on the resident matrix, {time.time() - t0:.2f} s: held-out loss per unit of exposure")
    for lam, mean, se in zip(cv.lams, cv.mean, cv.se):
        mark = "  <- best" if lam == cv.lam_best else ("  <- 1 se" if lam == cv.lam_1se else "")
        print(f"{lam / lam_max:14.5f} {mean:14.8f} +- {se:.2e}{mark}")


if __name__ == "__main__":
    main()
